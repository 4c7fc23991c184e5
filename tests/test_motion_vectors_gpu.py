"""Motion vectors for deforming meshes (hk_set_mesh_motion_vectors; DESIGN 4 "Motion vectors for deforming meshes").  The scene, the float64
restatement of a pixel's velocity and the reprojection check live in motion_vectors_ref.py: a 5 x 5-vertex grid G (32 triangles) instanced
twice - G1 at rest, G2 posed anew every frame - a quad S behind them (posed anew every frame: the rigid baseline), one emissive quad, a
generic camera that drifts, 76 x 44 pixels (no multiple of the 8 x 8 tiles).

The tolerance of the float64 comparisons is not a constant of this file: the same restatement with previous = current vertices is applied
to S's pixels of the same frame, whose velocity the unchanged rigid code of the prepass wrote; its largest absolute error is e0 and the
deforming pixels must agree within 4 e0 (three more interpolations, and barycentrics recovered from a rounded position)."""
import functools

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from cases import diff_buffers, product_default_traversal, snapshot

import motion_vectors_ref as R

pytestmark = pytest.mark.gpu

EXACT = F.CTX_DETERMINISTIC_SCATTER   # (with the suite's HK_CTX_EXACT_TRAVERSAL: tests/conftest.py)


def settings(**more):
    return hk.HikariSettings(**dict(R.SETTINGS, **more))


class Run:
    """one context with its own copy of the scene"""

    def __init__(self, enable, cells=4, flags=EXACT, default_traversal=False, filler=False, count=False):
        self.ms = R.MotionScene(cells, filler)
        if default_traversal:
            with product_default_traversal():
                self.p = hk.HikariPlugin(device=0, flags=flags)
        else:
            self.p = hk.HikariPlugin(device=0, flags=flags)
        self.p.set_scene(self.ms.scene)
        if count:
            self.p.engine.set_debug_option(F.DEBUG_OPT_MOTION_COUNT, 1)
        if enable:
            self.p.set_mesh_motion_vectors(self.ms.index)
        self.views = {}

    def deform(self, positions, normals):
        self.p.deform_meshes([("vertices", self.ms.index, positions, normals)])
        self.ms.current = np.asarray(positions, np.float32).copy()

    def frame(self, n, s=None, move=True):
        if move and n > 1:
            self.ms.move(self.p.engine, n)
        cam, before = R.camera(n), self.p._previous_camera
        self.views[n] = (cam.view_uniform(), cam.previous_view_uniform(before))
        self.p.render(cam, s or settings(), frame_number=n)
        self.previous_of_frame = self.ms.previous.copy()
        self.ms.frame_done()

    def read(self, buf):
        return self.p.engine.read(buf)


def same_frame(a, b, what):
    bad = diff_buffers(snapshot(a.p), snapshot(b.p))
    assert bad == {}, f"{what}: {bad}"


def compare_with_float64(run, n, what):
    """case 3's comparison on frame n of `run` (just rendered): returns the figures, asserts the bound"""
    ms = run.ms
    pos, im, vel = run.read(F.BUF_POSITION), run.read(F.BUF_INSTANCE_MATERIAL), run.read(F.BUF_VELOCITY_UV)
    view, pview = run.views[n]
    s_ids = [i for i, k in enumerate(ms.kind) if k == "S"]
    g_ids = [i for i, k in enumerate(ms.kind) if k == "G"]
    e0, s_pixels, s_margin = 0.0, 0, 1.0
    for i in s_ids:   # the restatement's own error, on the parent's rigid code
        px = R.pixels_of(im, [i])
        v, _, margin, _ = R.restate(pos, px, ms.poses[i][0], ms.poses[i][1], ms.s_positions, ms.s_positions, ms.s_indices, view, pview)
        keep = margin >= R.EDGE_MARGIN
        e0 = max(e0, float(np.abs(v - vel[px[0], px[1], :2].astype(np.float64))[keep].max()))
        s_pixels += len(px[0])
        s_margin = min(s_margin, float(keep.mean()))
    out = dict(e0=e0, s_pixels=s_pixels, worst=0.0, pixels=0, left_out=0, moved=0)
    for i in g_ids:
        px = R.pixels_of(im, [i])
        got = vel[px[0], px[1], :2].astype(np.float64)
        v, _, margin, _ = R.restate(pos, px, ms.poses[i][0], ms.poses[i][1], ms.current, run.previous_of_frame, ms.indices, view, pview)
        rigid, _, _, _ = R.restate(pos, px, ms.poses[i][0], ms.poses[i][1], ms.current, ms.current, ms.indices, view, pview)
        keep = margin >= R.EDGE_MARGIN
        err = np.abs(v - got).max(axis=1)
        out["worst"] = max(out["worst"], float(err[keep].max()))
        out["pixels"] += len(px[0])
        out["left_out"] += int((~keep).sum())
        out["moved"] += int((np.abs(got - rigid).max(axis=1) > 4.0 * e0).sum())
    print(what, out)
    if s_ids:
        assert s_pixels >= 200 and s_margin >= 0.98, (what, out)   # (the camera keeps the parent's own pixels inside the edge condition)
        assert e0 > 0.0
    assert out["pixels"] >= 100, (what, out)
    assert out["left_out"] <= 0.02 * out["pixels"], (what, out)
    if s_ids:
        assert out["worst"] <= 4.0 * e0, (what, out)
    assert out["moved"] >= 0.5 * out["pixels"], (what, "the velocity equals the rigid formula's on most pixels: the comparison shows nothing", out)
    return out


# ---- 1
def test_identity_is_invisible():
    """A enables motion on G and, before each of 4 frames, sends G's unchanged vertices through HK_DEFORM_VERTICES; twin B does the same
    without enabling.  Every screen-space buffer is byte-equal in every frame (the pass runs - the mesh is live - and rewrites nothing)."""
    a, b = Run(True, count=True), Run(False)
    for n in range(1, 5):
        for r in (a, b):
            r.deform(r.ms.rest, r.ms.rest_normals)
            r.frame(n)
        same_frame(a, b, f"frame {n}")
        assert a.p.engine.last_motion() == (1, 1, 0), (n, a.p.engine.last_motion())
        assert b.p.engine.last_motion() == (0, 0, 0)


# ---- 2
def test_frame_rule():
    """Two deformations before frame 2 (to X, then to Y) leave `previous` at frame 1's state: all buffers of frame 2 equal those of a twin
    that deformed once, to Y.  Frame 3 follows with no deformation: no motion pass, and velocity_uv is a never-enabled twin's."""
    a, a1, never = Run(True), Run(True), Run(False)
    x, xn = R.displaced(a.ms.rest, 21)
    y, yn = R.displaced(a.ms.rest, 22)
    for r in (a, a1, never):
        r.frame(1)
    assert a.p.engine.last_motion()[:2] == (0, 0)
    a.deform(x, xn)
    for r in (a, a1, never):
        r.deform(y, yn)
        r.frame(2)
    same_frame(a, a1, "frame 2")
    assert a.p.engine.last_motion()[:2] == (1, 1) and a1.p.engine.last_motion()[:2] == (1, 1)
    moved = a.read(F.BUF_VELOCITY_UV).tobytes() != never.read(F.BUF_VELOCITY_UV).tobytes()
    assert moved, "frame 2's velocity equals the rigid one: the frame rule was not exercised"
    for r in (a, never):
        r.frame(3)
    assert a.p.engine.last_motion()[:2] == (0, 0)
    assert a.read(F.BUF_VELOCITY_UV).tobytes() == never.read(F.BUF_VELOCITY_UV).tobytes(), "a velocity lingers in a frame that follows no deformation"


# ---- 3
@functools.lru_cache(maxsize=None)
def x_to_y(cells, default_traversal):
    """G deformed to X before frame 1 and from X to Y between frames 1 and 2; the run after frame 2 (shared by cases 3 and 7, left unchanged)"""
    run = Run(True, cells=cells, flags=0 if default_traversal else EXACT, default_traversal=default_traversal, count=True)
    x, xn = R.displaced(run.ms.rest, 11)
    y, yn = R.displaced(run.ms.rest, 12)
    run.deform(x, xn)
    run.frame(1)
    run.deform(y, yn)
    run.frame(2)
    return run


@pytest.mark.parametrize("cells,default_traversal", [(4, False), (24, True)], ids=["lds_prepass", "wide_walk"])
def test_velocity_against_float64(cells, default_traversal):
    """Every pixel of frame 2 on G1 or G2 against the float64 restatement, within 4 e0 (e0: the same restatement on S's rigid pixels).
    Measured on one MI355X run: see DESIGN 4."""
    run = x_to_y(cells, default_traversal)
    if default_traversal:   # 1 152 triangles: the blob exceeds the LDS copy, the prepass is the wide walk
        assert run.p.engine.wide_walk() and run.p.engine.traversal_mode()[0] == "threaded", run.p.engine.traversal_mode()
    else:
        assert not run.p.engine.wide_walk()
    out = compare_with_float64(run, 2, f"velocity vs float64, {cells + 1} x {cells + 1} vertices")
    launches, live, rewritten = run.p.engine.last_motion()
    assert (launches, live) == (1, 1) and 0.5 * out["pixels"] <= rewritten <= out["pixels"], (launches, live, rewritten, out)


# ---- 4
def test_reprojection_lands_on_the_same_surface_point():
    """Frame 1's position plane at the nearest texel of uv - velocity, for frame 2's G1 pixels: within one pixel's footprint of the float64
    previous world point.  The rigid velocity fails the same check for most of them.  (No TAA jitter: the planes are sampled at texel centres.)"""
    run = Run(True)
    s = settings(taa=hk.Taa.NONE)
    x, xn = R.displaced(run.ms.rest, 11)
    y, yn = R.displaced(run.ms.rest, 12)
    run.deform(x, xn)
    run.frame(1, s)
    pos1, im1 = run.read(F.BUF_POSITION), run.read(F.BUF_INSTANCE_MATERIAL)
    run.deform(y, yn)
    run.frame(2, s)
    pos2, im2, vel = run.read(F.BUF_POSITION), run.read(F.BUF_INSTANCE_MATERIAL), run.read(F.BUF_VELOCITY_UV)
    ms, (view, pview) = run.ms, run.views[2]
    px = R.pixels_of(im2, [0])
    _, prev_world, _, _ = R.restate(pos2, px, ms.poses[0][0], ms.poses[0][1], y, x, ms.indices, view, pview)
    rigid, _, _, _ = R.restate(pos2, px, ms.poses[0][0], ms.poses[0][1], y, y, ms.indices, view, pview)
    with_feature = R.reprojection(px, vel[px[0], px[1], :2].astype(np.float64), prev_world, pos1, im1, im2, 0)
    with_rigid = R.reprojection(px, rigid, prev_world, pos1, im1, im2, 0)
    print("reprojection", with_feature, "rigid", with_rigid)
    assert with_feature["qualify"] >= 0.6 * with_feature["pixels"], with_feature
    assert with_feature["within"] == with_feature["qualify"], with_feature
    assert with_rigid["fail_of_own"] > 0.5 * with_rigid["own"], with_rigid


# ---- 5
def test_structure_edits_keep_it_right():
    """With motion live on G: hk_change_scene_instances removes S (ids shift) and adds a third instance of G; hk_remove_meshes removes a mesh
    with a lower id than G; hk_rebuild_mesh_tree runs on G.  After each, a deformation and a frame, compared as in case 3 (e0 from S while
    the scene has it, then the last e0 measured).  After disabling, the next frame's velocity is a never-enabled twin's.
    (The 25 x 25-vertex grid: hk_change_scene_instances after a deformation takes a scene beyond the LDS copy - one that keeps two slots
    of its instance level - and refuses the small one with HK_E_NOT_READY.)"""
    a, never = Run(True, cells=24, filler=True), Run(False, cells=24, filler=True)
    runs = (a, never)
    seeds = iter(range(31, 40))

    def step(n):
        for r in runs:
            p, q = R.displaced(r.ms.rest, seed)
            r.deform(p, q)
            r.frame(n)

    seed = next(seeds)
    step(1)
    seed = next(seeds)
    step(2)
    first = compare_with_float64(a, 2, "before the edits")
    e0 = first["e0"]

    def compare(n, what):
        out = compare_with_float64(a, n, what)
        assert out["worst"] <= 4.0 * e0, (what, out, e0)

    # -- the instance set: S leaves (the emissive quad's id shifts), a third instance of G arrives
    for r in runs:
        ms, b = r.ms, r.ms.builder
        b.remove_instance(2)
        b.add_instance(ms.g, ms.grey, R.g3_pose())
        ms.kind = ["G", "G", "E", "G"]
        ms.poses = [ms.poses[0], ms.poses[1], ms.poses[3], [R.g3_pose(), R.g3_pose()]]
        r.p.change_instances(b)
    seed = next(seeds)
    step(3)
    compare(3, "after hk_change_scene_instances")
    assert a.p.engine.last_motion()[:2] == (1, 1)
    # -- the mesh level: the filler (a lower mesh id than G) leaves, G's record is rebased
    for r in runs:
        ms, b = r.ms, r.ms.builder
        extent = b.remove_mesh(ms.filler)
        r.p.remove_meshes([extent])
        b.finish()
        ms.g -= 1
        old = bytes(ms.index)
        ms.index = b.mesh_index(ms.g)
        assert bytes(ms.index) != old
    seed = next(seeds)
    step(4)
    compare(4, "after hk_remove_meshes")
    # -- the tree: triangles may be visited in any order, the planes are keyed by vertex
    for r in runs:
        r.p.engine.rebuild_mesh_tree(r.ms.index, F.TREE_SAH)
    seed = next(seeds)
    step(5)
    compare(5, "after hk_rebuild_mesh_tree")
    # -- off again
    a.p.set_mesh_motion_vectors(a.ms.index, False)
    seed = next(seeds)
    step(6)
    assert a.p.engine.last_motion() == (0, 0, 0)
    assert a.read(F.BUF_VELOCITY_UV).tobytes() == never.read(F.BUF_VELOCITY_UV).tobytes()
    ga, gn = a.p.engine.read_mesh_geometry(a.ms.index), never.p.engine.read_mesh_geometry(never.ms.index)
    for key in ("positions", "normals", "triangles", "box"):
        assert ga[key].tobytes() == gn[key].tobytes(), key


# ---- 6
def grid_skin(rest):
    """two joints along x: every vertex follows both, by its x"""
    f = (rest[:, 0].astype(np.float64) / R.GRID_SIZE + 0.5)
    ji = np.zeros((len(rest), 4), np.uint16)
    ji[:, 1] = 1
    jw = np.zeros((len(rest), 4), np.float32)
    jw[:, 0], jw[:, 1] = 1.0 - f, f
    return ji, jw


def grid_joints(n):
    out = []
    for k in range(2):
        a = 0.25 * np.sin(0.9 * n + 1.3 * k)
        c, s = np.cos(a), np.sin(a)
        m = np.array([[c, -s, 0, 0.02 * n * k], [s, c, 0, 0.05 * k], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
        out.append(m.T.reshape(-1))
    return np.stack(out).astype(np.float32)


@pytest.mark.parametrize("source", ["skin", "morph_skin", "device_vertices"])
def test_every_source_of_vertices(source):
    """A drives G by HK_DEFORM_SKIN, by HK_DEFORM_MORPH_SKIN, or through hk_deform_meshes_device with recomputed normals; twin B gets the
    vertices A's device holds as HK_DEFORM_VERTICES items.  Both enabled: all buffers byte-equal over 3 frames."""
    a, b = Run(True), Run(True)
    ms = a.ms
    if source != "device_vertices":
        ji, jw = grid_skin(ms.rest)
        a.p.engine.set_mesh_skin(ms.index, ms.rest, ms.rest_normals, ji, jw)
    if source == "morph_skin":
        dp, dn = S.morph_targets(ms.rest, ms.rest_normals, 3, seed=5)
        a.p.engine.set_mesh_morph_targets(ms.index, ms.rest, ms.rest_normals, dp, dn)
    keep = []
    for n in range(1, 4):
        if source == "skin":
            a.p.deform_meshes([("skin", ms.index, grid_joints(n))])
        elif source == "morph_skin":
            a.p.deform_meshes([("morph_skin", ms.index, grid_joints(n), S.morph_weights(3, n, mode="all"))])
        else:
            import torch

            t = torch.from_numpy(R.displaced(ms.rest, 50 + n)[0]).to(torch.device("cuda", 0))
            keep.append(t)
            a.p.deform_meshes([("vertices", ms.index, t, None, dict(recompute_normals=True))])
        held = a.p.engine.read_mesh_geometry(ms.index)
        b.deform(held["positions"], held["normals"])
        for r in (a, b):
            r.frame(n)
        same_frame(a, b, f"{source}, frame {n}")
        assert a.p.engine.last_motion()[:2] == (1, 1) and a.p.engine.last_deform()[3] in (5, 6)


# ---- 7
def test_bands_equal_the_single_context():
    """hk_multi_* with 3 bands on one device over case 3's small scene: after hk_multi_set_mesh_motion_vectors and one deformation the merged
    velocity_uv and tone-mapped image equal the single context's byte for byte."""
    from bevy_hikari_amd.distributed import MultiEngine

    single = x_to_y(4, False)
    ms = R.MotionScene(4)
    m = MultiEngine([0, 0, 0])
    m.upload_noise()
    m.upload_scene(ms.scene)
    m.resize(R.W, R.H, 1.0)
    m.set_mesh_motion_vectors(ms.index)
    s = settings()
    x, xn = R.displaced(ms.rest, 11)
    y, yn = R.displaced(ms.rest, 12)
    lights = hk.lights_uniform()
    before = None
    for n, (p, q) in ((1, (x, xn)), (2, (y, yn))):
        if n > 1:
            for i, new in ((1, R.g2_pose(n)), (2, R.s_pose(n))):
                ms.builder.set_instance_transform(i, new)
            m.refit_instances(ms.builder)
        m.deform_meshes([("vertices", ms.index, p, q)])
        cam = R.camera(n)
        m.frame_render(hk.frame_uniform(s, n), cam.view_uniform(), cam.previous_view_uniform(before), lights, s.to_c())
        before = cam
    m.wait()
    for buf, name in ((F.BUF_VELOCITY_UV, "velocity_uv"), (F.BUF_TONE_MAPPED, "tone_mapped")):
        assert m.read(buf).tobytes() == single.read(buf).tobytes(), f"{name} of the bands' union differs from the single context's"
    for e in m.contexts:
        assert e.last_motion()[:2] == (1, 1)
