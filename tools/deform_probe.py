#!/usr/bin/env python3
"""Mesh deformation: the host path (hk_scene_builder_set_mesh_vertices + finish + hk_upload_scene: the reference's re-prepared mesh,
mesh.rs:76-166) against the device path (hk_update_mesh_vertices / hk_skin_mesh: vertices, triangles, the mesh tree refit in every
ordering, the instance level) for one cloth mesh of ~10^4 / 10^5 / 10^6 triangles in a scene beyond the LDS copy (eight orderings).
Device times: host wall clock of the call plus the wait for everything it enqueued (hk_debug_read_emitters flushes and synchronises),
median of the repeats.  Also the SAH cost (node area / root area, summed) of the refit tree against a fresh host build over the same
deformed triangles; then the fold (rebuild_probe): a deformation a refit handles badly, and hk_rebuild_mesh_tree against it.   Usage: python tools/deform_probe.py [--out FILE] [triangles ...]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder, standard_material


def sah_cost(nodes, count, offset=0):
    """sum of navigator and leaf box areas over the root's, for the mesh tree in nodes[offset:offset+count] (leaf boxes filled in)"""
    a = np.frombuffer(bytes(nodes), dtype=np.float32).reshape(-1, 8)[offset:offset + count]
    lo, hi = a[:, 0:3].astype(np.float64), a[:, 4:7].astype(np.float64)
    d = np.maximum(hi - lo, 0.0)
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    root = np.maximum(hi.max(axis=0) - lo.min(axis=0), 0.0)
    return float(area.sum() / (root[0] * root[1] + root[1] * root[2] + root[2] * root[0]))


def sync(engine):
    n, m = F.u32(), F.u32()
    engine.api.call("debug_read_emitters", engine.ctx, None, 0, C.byref(n), None, 0, C.byref(m))


def probe(triangles, repeats=10):
    p, n, uv, idx = S.large_cloth(triangles)
    scene, sun = S.synthetic_scene(n_boxes=20, n_spheres=5, n_emitters=2, sphere_rings=12, sphere_segs=16)
    b = scene.builder
    t0 = time.perf_counter()
    mid = b.add_mesh(p, n, uv, idx)
    add_ms = 1e3 * (time.perf_counter() - t0)
    b.add_instance(mid, b.add_material(standard_material((0.7, 0.2, 0.2, 1.0), (0, 0, 0), 0.7, 0.0, 0.5)), np.eye(4, dtype=np.float32).reshape(-1))
    scene = b.finish()
    index = b.mesh_index(mid)
    eng = hk.Engine(device=0, flags=0)
    eng.upload_noise()
    eng.upload_scene(scene)
    sync(eng)
    out = {"triangles": len(idx) // 3, "vertices": len(p), "host_bvh_build_ms": round(add_ms, 2)}
    mode, orderings = C.c_uint32(), C.c_uint32()
    eng.api.call("traversal_mode", eng.ctx, C.byref(mode), C.byref(orderings))
    out["orderings"] = orderings.value
    # host path: the builder mirrors the change, the scene goes up again (the mesh level is laid out on the host)
    host = []
    for r in range(3):
        q, qn = S.waving_cloth(p, r + 1, amplitude=0.3)
        t0 = time.perf_counter()
        b.set_mesh_vertices(mid, q, qn)
        new = b.finish()
        eng.upload_scene(new)
        sync(eng)
        host.append(1e3 * (time.perf_counter() - t0))
    out["host_path_ms"] = round(float(np.median(host)), 2)
    # device path: hk_update_mesh_vertices, then everything it enqueued
    dev = []
    for r in range(repeats):
        q, qn = S.waving_cloth(p, r + 10, amplitude=0.3)
        t0 = time.perf_counter()
        eng.update_mesh_vertices(index, q, qn)
        sync(eng)
        dev.append(1e3 * (time.perf_counter() - t0))
    out["device_update_ms"] = round(float(np.median(dev)), 3)
    # skinning: two joints along x
    ji = np.zeros((len(p), 4), np.uint16)
    ji[:, 1] = 1
    w = np.zeros((len(p), 4), np.float32)
    w[:, 1] = (p[:, 0] + 1.0) / 2.0
    w[:, 0] = 1.0 - w[:, 1]
    eng.set_mesh_skin(index, p, n, ji, w)
    skin = []
    for r in range(repeats):
        j = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (2, 1))
        j[1, 13] = 0.05 * r
        t0 = time.perf_counter()
        eng.skin_mesh(index, j)
        sync(eng)
        skin.append(1e3 * (time.perf_counter() - t0))
    out["device_skin_ms"] = round(float(np.median(skin)), 3)
    # refit quality: the refit tree after a large deformation against a fresh host build over the same triangles
    q, qn = S.waving_cloth(p, 7, amplitude=0.6)
    eng.update_mesh_vertices(index, q, qn)
    nodes, count, o = eng.read_mesh_nodes()
    out["sah_refit"] = round(sah_cost(nodes, index.node_count, index.node_offset), 3)
    fresh = SceneBuilder()
    fid = fresh.add_mesh(q, qn, uv, idx)
    fresh.add_instance(fid, fresh.add_material(standard_material()), np.eye(4, dtype=np.float32).reshape(-1))
    f = fresh.finish()
    fe = hk.Engine(device=0, flags=F.CTX_EXACT_TRAVERSAL)
    fe.upload_scene(f)
    fn, fc, _ = fe.read_mesh_nodes()
    out["sah_fresh_build"] = round(sah_cost(fn, fc), 3)
    fe.close()
    rebuild_probe(eng, index, p, uv, idx, out, sun)
    eng.close()
    return out


def frame_ms(eng, sun, frames=8, warmup=6, size=(960, 540), first=1):
    """mean time of `frames` frames looking at the scene's middle (where the cloth lies) after `warmup` frames, host wall clock; the same
    frame numbers for every tree (the caller resizes once)"""
    from bevy_hikari_amd.plugin import Camera, look_at_transform

    cam = Camera(look_at_transform((0.0, 2.0, 2.4), (0.0, 0.0, 0.0)), *size)   # (the cloth lies around the origin)
    lights, s = hk.lights_uniform(directional=sun), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    for n in range(first, first + warmup):
        eng.frame_render(hk.frame_uniform(s, n), view, pview, lights, s.to_c())
    eng.wait()
    t0 = time.perf_counter()
    for n in range(first + warmup, first + warmup + frames):
        eng.frame_render(hk.frame_uniform(s, n), view, pview, lights, s.to_c())
    eng.wait()
    return round(1e3 * (time.perf_counter() - t0) / frames, 3)


def rebuild_probe(eng, index, rest, uv, idx, out, sun, repeats=5):
    """A deformation a refit handles badly - the cloth folded onto itself along its middle line (S.folded_cloth) - and the rebuild of its
    tree on the device (hk_rebuild_mesh_tree): SAH cost of the refit tree, of the rebuilt tree and of a fresh host build, the time of the
    rebuild (call + flush + full synchronisation), and of a frame with either tree; the same for HK_TREE_LBVH."""
    q, qn = S.folded_cloth(rest)
    cost = lambda: round(sah_cost(eng.read_mesh_nodes()[0], index.node_count, index.node_offset), 3)

    def refit_state():   # the device's tree still has the bind pose's shape (only refits so far): deforming refits it to the fold
        eng.update_mesh_vertices(index, q, qn)
        sync(eng)

    eng.resize(960, 540, 1.0)
    refit_state()
    out["fold_sah_refit"] = cost()
    out["fold_frame_refit_ms"] = frame_ms(eng, sun)
    fresh = SceneBuilder()
    t0 = time.perf_counter()
    fid = fresh.add_mesh(q, qn, uv, idx)
    out["fold_host_bvh_build_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    fresh.add_instance(fid, fresh.add_material(standard_material()), np.eye(4, dtype=np.float32).reshape(-1))
    fe = hk.Engine(device=0, flags=F.CTX_EXACT_TRAVERSAL)
    fe.upload_scene(fresh.finish())
    fn, fc, _ = fe.read_mesh_nodes()
    out["fold_sah_fresh_build"] = round(sah_cost(fn, fc), 3)
    fe.close()
    times = []
    for r in range(repeats):   # (the first call grows the scratch: the median leaves it out)
        t0 = time.perf_counter()
        eng.rebuild_mesh_tree(index, F.TREE_SAH)
        sync(eng)
        eng.wait()
        times.append(1e3 * (time.perf_counter() - t0))
    out["device_rebuild_ms"] = round(float(np.median(times)), 3)
    out["fold_sah_device_rebuild"] = cost()
    out["fold_frame_rebuilt_ms"] = frame_ms(eng, sun)
    if out["triangles"] <= 200_000:   # once: the top of the build in one workgroup, as the instance tree's build runs it
        eng.set_debug_option(F.DEBUG_OPT_MESH_REBUILD_ONE_WORKGROUP, 1)
        times = []
        for r in range(3):
            t0 = time.perf_counter()
            eng.rebuild_mesh_tree(index, F.TREE_SAH)
            sync(eng)
            eng.wait()
            times.append(1e3 * (time.perf_counter() - t0))
        out["device_rebuild_one_workgroup_top_ms"] = round(float(np.median(times)), 3)
        eng.set_debug_option(F.DEBUG_OPT_MESH_REBUILD_ONE_WORKGROUP, 0)
    times = []
    for r in range(repeats):
        t0 = time.perf_counter()
        eng.rebuild_mesh_tree(index, F.TREE_LBVH)
        sync(eng)
        eng.wait()
        times.append(1e3 * (time.perf_counter() - t0))
    out["device_rebuild_lbvh_ms"] = round(float(np.median(times)), 3)
    out["fold_sah_lbvh"] = cost()
    out["fold_frame_lbvh_ms"] = frame_ms(eng, sun)
    out["rebuild_over_host_build"] = round(out["device_rebuild_ms"] / out["fold_host_bvh_build_ms"], 4)
    out["rebuild_over_device_update"] = round(out["device_rebuild_ms"] / out["device_update_ms"], 2)


if __name__ == "__main__":
    args = sys.argv[1:]
    path = None
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    sizes = [int(a) for a in args] or [10_000, 100_000, 1_000_000]
    rows = []
    for t in sizes:
        r = probe(t)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if path:
        with open(path, "w") as fh:
            json.dump({"probe": "tools/deform_probe.py", "rows": rows}, fh, indent=1)
