"""Shared by tests/test_motion_vectors_gpu.py: the scene of the motion-vector tests (a 5x5-vertex grid G instanced twice - G1 at rest, G2
posed anew every frame - a quad S behind them, posed anew every frame too, one emissive quad, a camera at a generic place, 76 x 44
pixels) and the float64 restatement of a pixel's velocity from the stored world position:

    local      = inverse(model) * stored world position
    triangle   = the triangle of the CURRENT vertices that contains it, with its barycentrics (u, v)
    previous   = previous model * (P0 + u (P1 - P0) + v (P2 - P0)),  P = the PREVIOUS vertices of that triangle
    velocity   = clip_to_uv(view_proj * world) - clip_to_uv(previous_view_proj * previous)

with the two view-projection matrices as the frame's float32 uniforms hold them.  With previous vertices = current vertices this is the
rigid formula the prepass has always used, which is how the tests measure the restatement's own error on S."""
import math

import numpy as np

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder, standard_material

W, H = 76, 44
SETTINGS = dict(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
GRID_SIZE = 2.0
EDGE_MARGIN = 1e-4   # barycentric units: pixels nearer to a triangle edge than this may be left out


def camera(n=0):
    """the frame's camera: non-round eye and target, drifting a little from frame to frame (so that the previous view-projection matters)"""
    return hk.Camera(hk.look_at_transform((0.797 + 0.011 * n, 2.043 + 0.007 * n, 2.371 - 0.005 * n), (0.071, 0.113, -0.047)), W, H)


def g1_pose():
    return S._trs((-0.35, 0.0, 0.25), (0.05, 0.2, -0.04), (1.0, 1.0, 1.0))


def g2_pose(n):
    return S._trs((1.55 + 0.03 * n, 0.45 + 0.02 * n, -0.9), (0.3, -0.5 + 0.04 * n, 0.2), (0.55, 0.55, 0.55))


def g3_pose():
    return S._trs((-1.6, 0.6, -1.2), (0.6, 0.3, 0.0), (0.5, 0.5, 0.5))


def s_pose(n):
    return S._trs((0.2 + 0.04 * n, -0.6, -0.4 - 0.02 * n), (0.0, 0.1 + 0.03 * n, 0.0), (7.0, 1.0, 7.0))


def e_pose():
    return S._trs((0.3, 3.4, 0.2), (math.pi, 0.3, 0.0), (1.5, 1.0, 1.5))


def displaced(rest, seed, amount=0.1 * GRID_SIZE):
    """a seeded smooth displacement of the grid's vertices, of the order of a tenth of the grid's size; normals from the height field"""
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(0.6, 1.0, 3) * amount
    kx, kz, px, pz = rng.uniform(1.5, 3.0), rng.uniform(1.5, 3.0), rng.uniform(0, 6.28), rng.uniform(0, 6.28)
    x, z = rest[:, 0].astype(np.float64), rest[:, 2].astype(np.float64)
    p = rest.astype(np.float64).copy()
    p[:, 1] += a * np.sin(kx * x + px) * np.cos(kz * z + pz)
    p[:, 0] += 0.5 * b * np.sin(kz * z + px)
    p[:, 2] += 0.5 * c * np.cos(kx * x + pz)
    dx = a * kx * np.cos(kx * x + px) * np.cos(kz * z + pz)
    dz = -a * kz * np.sin(kx * x + px) * np.sin(kz * z + pz)
    n = np.stack([-dx, np.ones_like(dx), -dz], -1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p.astype(np.float32), n.astype(np.float32)


class MotionScene:
    """builder, scene and the host's book-keeping of one context's copy of the scene"""

    def __init__(self, cells=4, filler=False):
        b = SceneBuilder()
        self.builder = b
        self.filler = b.add_mesh(*S._box(0.3, 0.3, 0.3)) if filler else None   # (a mesh with a lower id than G that no instance uses)
        gp, gn, guv, gidx = S.cloth_grid(cells, cells, size=GRID_SIZE)
        self.rest, self.rest_normals, self.indices = gp, gn, gidx.reshape(-1, 3)
        self.g = b.add_mesh(gp, gn, guv, gidx)
        qp, qn, quv, qidx = S.cloth_grid(1, 1, size=1.0)
        self.s_positions, self.s_indices = qp, qidx.reshape(-1, 3)
        self.s = b.add_mesh(qp, qn, quv, qidx)
        self.e = b.add_mesh(qp, qn, quv, qidx)
        grey = b.add_material(standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
        blue = b.add_material(standard_material((0.3, 0.5, 0.8, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
        glow = b.add_material(standard_material((0.9, 0.9, 0.9, 1.0), (4.0, 3.6, 3.0), 1.0, 0.0, 0.5))
        self.grey = grey
        # instance ids in this order; poses[i] = (current model, previous model) as float32[16] column-major, kind[i] in "G", "S", "E"
        self.kind = ["G", "G", "S", "E"]
        self.poses = []
        for mesh, mat, pose in ((self.g, grey, g1_pose()), (self.g, blue, g2_pose(0)), (self.s, blue, s_pose(0)), (self.e, glow, e_pose())):
            b.add_instance(mesh, mat, pose)
            self.poses.append([pose, pose])
        self.scene = b.finish()
        self.scene.builder = b
        self.index = b.mesh_index(self.g)
        self.current = gp.copy()    # G's vertices as the device holds them, and those it held when the last frame's rays were enqueued
        self.previous = gp.copy()

    def move(self, engine, n):
        """frame n's poses of G2 and S (where the scene still has them) through hk_refit_scene_instances"""
        for i, kind in enumerate(self.kind):
            new = g2_pose(n) if (kind == "G" and i == 1) else s_pose(n) if kind == "S" else None
            self.poses[i][1] = self.poses[i][0]
            if new is not None:
                self.builder.set_instance_transform(i, new)
                self.poses[i][0] = new
        engine.refit_instances(self.builder)

    def frame_done(self):
        self.previous = self.current.copy()


def mat4(m):
    return np.asarray(m, np.float32).reshape(4, 4).T.astype(np.float64)


def clip_to_uv(clip):
    uv = (clip[..., :2] / clip[..., 3:4] + 1.0) * 0.5
    uv[..., 1] = 1.0 - uv[..., 1]
    return uv


def locate(local, vertices, indices):
    """per point: (triangle, u, v, margin) - the triangle of `vertices` that contains it (nearest to its plane among those that do), its
    barycentrics and their distance from the nearest edge, all float64"""
    tri = vertices.astype(np.float64)[indices]                    # [t][3][3]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = local[:, None, :] - a[None, :, :]                         # [p][t][3]
    g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    det = g11 * g22 - g12 * g12
    b1, b2 = (d * e1[None]).sum(-1), (d * e2[None]).sum(-1)
    u = (g22 * b1 - g12 * b2) / det
    v = (g11 * b2 - g12 * b1) / det
    off = np.abs((d * nrm[None]).sum(-1))
    margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
    cost = np.where(margin >= -1e-6, off, np.inf)
    t = np.argmin(cost, axis=1)
    k = np.arange(len(local))
    return t, u[k, t], v[k, t], margin[k, t], off[k, t]


def restate(position, pixels, model, previous_model, current, previous, indices, view, pview):
    """float64 velocity of `pixels` (ys, xs) of one instance: (velocity [n][2], previous world [n][3], margin [n], distance from the plane [n])"""
    ys, xs = pixels
    world = position[ys, xs, :3].astype(np.float64)
    m, pm = mat4(model), mat4(previous_model)
    local = np.concatenate([world, np.ones((len(world), 1))], 1) @ np.linalg.inv(m).T
    local = local[:, :3] / local[:, 3:4]
    t, u, v, margin, off = locate(local, current, indices)
    p = previous.astype(np.float64)[indices[t]]
    prev_local = p[:, 0] + u[:, None] * (p[:, 1] - p[:, 0]) + v[:, None] * (p[:, 2] - p[:, 0])
    prev_world = np.concatenate([prev_local, np.ones((len(world), 1))], 1) @ pm.T
    vp, pvp = mat4(view.view_proj), mat4(pview.view_proj)
    clip = np.concatenate([world, np.ones((len(world), 1))], 1) @ vp.T
    velocity = clip_to_uv(clip) - clip_to_uv(prev_world @ pvp.T)
    return velocity, prev_world[:, :3] / prev_world[:, 3:4], margin, off


def pixels_of(instance_material, ids):
    inst = np.floor(instance_material[..., 0]).astype(np.int64)
    hit = instance_material[..., 0] > 0.0
    return np.nonzero(hit & np.isin(inst, list(ids)))


def all3x3(mask):
    """where the pixel and its eight neighbours all lie in `mask` (the image's border never does)"""
    m = np.pad(mask, 1, constant_values=False)
    out = np.ones_like(mask)
    for dy in range(3):
        for dx in range(3):
            out &= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def reprojection(px, velocity, prev_world, pos1, im1, im2, instance):
    """Frame 1's position plane sampled at the nearest texel of uv - velocity for frame 2's pixels `px` of `instance`.  Examined: pixels whose
    3 x 3 neighbourhood is all that instance in both frames and whose sampled texel's is in frame 1.  Such a sample must lie within one
    pixel's world-space footprint of the float64 previous world point - the footprint being the largest distance between the sampled
    texel's world position and its eight neighbours' (the exact reprojected point lies within half a texel of the sampled one's centre).
    Returns the counts: pixels, own (both neighbourhoods), qualify, within."""
    ys, xs = px
    g1 = all3x3((im1[..., 0] > 0) & (np.floor(im1[..., 0]) == instance))
    g2 = all3x3((im2[..., 0] > 0) & (np.floor(im2[..., 0]) == instance))
    uv = np.stack([(xs + 0.5) / W, (ys + 0.5) / H], 1) - velocity
    tx, ty = np.floor(uv[:, 0] * W).astype(int), np.floor(uv[:, 1] * H).astype(int)
    inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
    own = g2[ys, xs] & g1[ys, xs]
    ok = own & inside & g1[tyc, txc]
    sample = pos1[tyc, txc, :3].astype(np.float64)
    foot = np.zeros(len(ys))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            n = pos1[np.clip(tyc + dy, 0, H - 1), np.clip(txc + dx, 0, W - 1), :3].astype(np.float64)
            foot = np.maximum(foot, np.linalg.norm(n - sample, axis=1))
    dist = np.linalg.norm(sample - prev_world, axis=1)
    return dict(pixels=len(ys), own=int(own.sum()), qualify=int(ok.sum()), within=int((ok & (dist <= foot)).sum()), worst=float((dist / np.maximum(foot, 1e-30))[ok].max()) if ok.any() else None,
                fail_of_own=int((own & ~(ok & (dist <= foot))).sum()))
