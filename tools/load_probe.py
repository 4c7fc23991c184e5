#!/usr/bin/env python3
"""Scene load: the host path (hk_scene_builder_add_mesh + finish + hk_upload_scene: `bvh` 0.7.1 BVH::build per mesh on one CPU thread)
against hk_load_scene (the meshes added DEFERRED, their trees built on the device) in HK_TREE_SAH and HK_TREE_LBVH, from the creation
of the builder to the end of the first frame's hk_frame_wait - one process per scene, the three paths one after the other in it, each on
a context of its own.  Per path: the host's tree builds (inside add_mesh), the rest of the builder's work, and for the loads where the
call's time went (hk_debug_last_load_times: mirrors, layout + upload, device build, read-back).  Then the check that the loaded scene
renders at the uploaded scene's speed: two more contexts, created after the three timed ones (a process's FIRST context renders faster
than its later ones, DESIGN 4 "Two streams": the timed paths' own frames are not comparable) - the twin builder (add_mesh +
hk_scene_builder_rebuild_mesh_tree) uploaded, the deferred builder loaded - whose mesh-level nodes must be the same bytes and whose
frames are timed alternately.  Not part of bench.py.
Usage: python tools/load_probe.py [--out FILE] [scene ...]      scenes: mesh_1e4 mesh_1e5 mesh_1e6 many_meshes flight_helmet"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import Camera, SceneBuilder, look_at_transform, standard_material

SCENES = ("mesh_1e4", "mesh_1e5", "mesh_1e6", "many_meshes", "flight_helmet")
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)


class Meter:
    """SceneBuilder.add_mesh timed, and deferred on request, while a scene is put together"""

    def __init__(self, deferred, twin=False):
        self.deferred, self.twin, self.add_ms, self.meshes = deferred, twin, 0.0, 0

    def __enter__(self):
        self.plain = SceneBuilder.add_mesh
        meter = self

        def add_mesh(builder, positions, normals, uvs, indices=None, topology=F.TOPOLOGY_TRIANGLE_LIST, build_tree=True):
            t0 = time.perf_counter()
            mesh = meter.plain(builder, positions, normals, uvs, indices, topology, build_tree=not meter.deferred)
            if meter.twin:
                builder.rebuild_mesh_tree(mesh)
            meter.add_ms += 1e3 * (time.perf_counter() - t0)
            meter.meshes += 1
            return mesh

        SceneBuilder.add_mesh = add_mesh
        return self

    def __exit__(self, *exc):
        SceneBuilder.add_mesh = self.plain


def one_mesh(triangles):
    def make():
        p, n, uv, idx = S.large_cloth(triangles)
        b = SceneBuilder()
        mat = b.add_material(standard_material((0.7, 0.2, 0.2, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
        lamp = b.add_material(standard_material((0.8, 0.8, 0.8, 1.0), (1.0, 0.95, 0.85), 1.0, 0.0, 0.5))
        b.add_instance(b.add_mesh(p, n, uv, idx), mat, IDENTITY)
        qp, qn, quv, qi = S.cloth_grid(1, 1, size=0.5)
        b.add_instance(b.add_mesh(qp, qn, quv, qi), lamp, S._trs((0.0, 1.5, 0.0), (np.pi, 0.0, 0.0), (1.0, 1.0, 1.0)))
        b.finish()
        return b, [], dict(color=(1.0, 0.96, 0.9), illuminance=15000.0, direction_to_light=(0.4, 0.8, 0.5)), Camera(look_at_transform((0.0, 2.0, 2.4), (0.0, 0.0, 0.0)), 960, 540)

    return make


def many_meshes(count=2000, rings=15, segs=25):
    """about 2 000 distinct meshes of 750 triangles each (rings x segs spheres, every one with radii of its own), one instance each"""
    def make():
        rng = np.random.default_rng(4)
        b = SceneBuilder()
        mat = b.add_material(standard_material((0.6, 0.6, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
        lamp = b.add_material(standard_material((0.8, 0.8, 0.8, 1.0), (1.0, 0.95, 0.85), 1.0, 0.0, 0.5))
        p, n, uv, idx = S._sphere(rings, segs)
        side = int(np.ceil(count ** 0.5))
        for k in range(count):
            q = (p * rng.uniform(0.6, 1.4, 3).astype(np.float32)).astype(np.float32)
            m = b.add_mesh(q, n, uv, idx)
            b.add_instance(m, lamp if k % 97 == 0 else mat, S._trs((2.5 * (k % side - side / 2), 0.0, 2.5 * (k // side - side / 2)), (0.0, 0.1 * k, 0.0), (1.0, 1.0, 1.0)))
        b.finish()
        return b, [], dict(color=(1.0, 0.96, 0.9), illuminance=15000.0, direction_to_light=(0.4, 0.8, 0.5)), \
            Camera(look_at_transform((0.0, 30.0, 1.6 * side), (0.0, 0.0, 0.0)), 960, 540)

    return make


def flight_helmet():
    def make():
        scene, sun, camera = S.flight_helmet_scene()
        return scene.builder, scene.textures, sun, camera(960, 540)

    return make


MAKERS = {"mesh_1e4": one_mesh(10_000), "mesh_1e5": one_mesh(100_000), "mesh_1e6": one_mesh(1_000_000), "many_meshes": many_meshes(), "flight_helmet": flight_helmet()}


def frames_ms(eng, cam, sun, first, frames=8, warmup=4):
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


def run_path(name, path):
    """one path, from the creation of the builder to the end of the first frame: a dict of times (ms), and the engine for the frame check"""
    make = MAKERS[name]
    eng = hk.Engine(device=0, flags=0)
    eng.upload_noise()
    eng.resize(960, 540, 1.0)
    eng.wait()
    t_start = time.perf_counter()
    with Meter(deferred=path != "upload") as meter:
        b, textures, sun, cam = make()
    t_built = time.perf_counter()
    if path == "upload":
        eng.upload_textures(textures)
        eng.api.call("upload_scene", eng.ctx, b.h)
        eng.traversal_mode()   # (the layout and its upload happen at the first use of the scene)
    else:
        eng.load_scene(b, F.TREE_SAH if path == "load_sah" else F.TREE_LBVH, textures)
    t_up = time.perf_counter()
    lights, s = hk.lights_uniform(directional=sun), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    eng.frame_render(hk.frame_uniform(s, 1), cam.view_uniform(), cam.previous_view_uniform(), lights, s.to_c())
    eng.wait()
    t_end = time.perf_counter()
    out = {"total_ms": round(1e3 * (t_end - t_start), 2), "add_mesh_ms": round(meter.add_ms, 2),
           "builder_other_ms": round(1e3 * (t_built - t_start) - meter.add_ms, 2), "upload_or_load_call_ms": round(1e3 * (t_up - t_built), 2),
           "first_frame_ms": round(1e3 * (t_end - t_up), 2)}
    if path != "upload":
        ms = (C.c_double * 5)()
        eng.api.call("debug_last_load_times", eng.ctx, ms)
        meshes, tris, launches, on_host = eng.last_load()
        out.update(mirrors_ms=round(ms[1], 2), layout_and_upload_ms=round(ms[2], 2), device_build_ms=round(ms[3], 3), readback_ms=round(ms[4], 2),
                   host_completion_ms=round(ms[0], 2), device_meshes=meshes, device_triangles=tris, build_launches=launches, host_meshes=on_host)
    _, count, orderings = eng.read_mesh_nodes()
    eng.close()
    return out, (meter.meshes, count, orderings)


def frame_check(name):
    """the uploaded twin and the loaded scene on two contexts of the same standing: node bytes, and frame times taken alternately"""
    engines = []
    for loaded in (False, True):
        eng = hk.Engine(device=0, flags=0)
        eng.upload_noise()
        eng.resize(960, 540, 1.0)
        with Meter(deferred=loaded, twin=not loaded):
            b, textures, sun, cam = MAKERS[name]()
        if loaded:
            eng.load_scene(b, F.TREE_SAH, textures)
        else:
            eng.upload_textures(textures)
            eng.api.call("upload_scene", eng.ctx, b.h)
        engines.append(eng)
    same = bytes(engines[0].read_mesh_nodes()[0]) == bytes(engines[1].read_mesh_nodes()[0])
    ms = [[], []]
    for r in range(3):
        for k, eng in enumerate(engines):
            ms[k].append(frames_ms(eng, cam, sun, 1 + 12 * r))
    for eng in engines:
        eng.close()
    return same, min(ms[0]), min(ms[1])


def child(name):
    res = {"scene": name}
    for path in ("upload", "load_sah", "load_lbvh"):
        res[path], (meshes, count, orderings) = run_path(name, path)
    res.update(meshes=meshes, mesh_nodes=count, orderings=orderings)
    res["load_sah_over_upload"] = round(res["load_sah"]["total_ms"] / res["upload"]["total_ms"], 3)
    res["load_lbvh_over_upload"] = round(res["load_lbvh"]["total_ms"] / res["upload"]["total_ms"], 3)
    same, up_ms, load_ms = frame_check(name)
    res.update(loaded_nodes_equal_uploaded_twin=same, frame_ms_uploaded_twin=up_ms, frame_ms_loaded=load_ms, frame_ms_loaded_over_uploaded=round(load_ms / up_ms, 3))
    print("RESULT " + json.dumps(res), flush=True)


def main(argv):
    if len(argv) >= 2 and argv[0] == "--child":
        return child(argv[1])
    out_path = os.path.join(ROOT, "profiles", "load_probe.json")
    if "--out" in argv:
        k = argv.index("--out")
        out_path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    results = []
    for name in argv or SCENES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout + r.stderr, file=sys.stderr)
            raise SystemExit(f"{name}: the probe failed")
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"what": "scene load from builder creation to the end of the first frame, ms: add_mesh + finish + hk_upload_scene against deferred meshes + hk_load_scene "
                   "(one run each, one process per scene; 960x540, one bounce)", "scenes": results}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
