#!/usr/bin/env python3
"""Meshes removed from a loaded scene: hk_remove_meshes against hk_load_scene of the remaining builder (the only route before it), in
the scenes of tools/add_mesh_probe.py - one mesh of 10^5 / 10^6 triangles (with twenty bystanders of 5 000 triangles that no instance
names, so that something can leave), 2 000 meshes of 750 - one process per (scene, shape).  Shapes: `one` mesh leaves, or every `tenth`.
In each process the scene is loaded with device-built trees and rendered; then, per entry:
  remove  the instances of the leaving meshes go (hk_update_scene_instances; many_meshes only), then hk_remove_meshes: the host time of
          the call, the time from the call to the end of the next frame, the compaction launch between two HIP events and its bytes
          (read + written: twice the bytes moved) over that time, next to hk_measure_hbm's copy rate of the same process
  load    hk_load_scene of the same, remaining builder in the same process state (the baseline: the full host layout)
and the device memory the process holds (hipMemGetInfo through torch) before the removal, after it, after the host has next waited for
every stream (the old allocation is freed there; the new one has the append's room, 1.5 times the survivors) and after the load.  One run per entry.  Not part of bench.py.
Usage: python tools/remove_mesh_probe.py [--out FILE] [scene ...]      scenes: mesh_1e5 mesh_1e6 many_meshes"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from load_probe import MAKERS, Meter

SCENES = ("mesh_1e5", "mesh_1e6", "many_meshes")
SHAPES = ("one", "tenth")
BYSTANDERS, BYSTANDER_TRIANGLES = 20, 5_000


def held_mb():
    import torch

    free, total = torch.cuda.mem_get_info(0)
    return round((total - free) / 2**20, 1)


def child(name, shape):
    eng = hk.Engine(device=0, flags=0)
    eng.upload_noise()
    eng.resize(960, 540, 1.0)
    with Meter(deferred=True):
        b, textures, sun, cam = MAKERS[name]()
        n_meshes = 2000 if name == "many_meshes" else 2
        if name != "many_meshes":
            p, n, uv, idx = S.large_cloth(BYSTANDER_TRIANGLES)
            for k in range(BYSTANDERS):
                b.add_mesh(p + 0.01 * k, n, uv, idx)
            n_meshes += BYSTANDERS
            b.finish()
    eng.load_scene(b, F.TREE_SAH, textures)
    lights, s = hk.lights_uniform(directional=sun), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    frame = [0]

    def render():
        frame[0] += 1
        eng.frame_render(hk.frame_uniform(s, frame[0]), view, pview, lights, s.to_c())

    for _ in range(4):
        render()
    eng.wait()
    _, nodes, orderings = eng.read_mesh_nodes()
    first = 0 if name == "many_meshes" else 2   # (the first mesh that may leave)
    leaving = [first + (n_meshes - first) // 2] if shape == "one" else list(range(first + 1, n_meshes, 10))
    res = {"scene": name, "shape": shape, "meshes": n_meshes, "meshes_removed": len(leaving), "scene_mesh_nodes": nodes, "orderings": orderings}
    res["held_before_mb"] = held_mb()
    builds = int(eng.stats().scene_mesh_builds)
    t0 = time.perf_counter()
    if name == "many_meshes":   # one instance per mesh, in mesh order
        for m in reversed(leaving):
            b.remove_instance(m)
        eng.update_instances_on_device(b, F.TREE_SAH)
    t1 = time.perf_counter()
    extents = [b.remove_mesh(m) for m in reversed(leaving)]
    t2 = time.perf_counter()
    eng.remove_meshes(extents)
    t3 = time.perf_counter()
    render()
    eng.wait()
    t4 = time.perf_counter()
    removed, tris, launches, runs, path, moved = eng.last_remove()
    launch_ms = eng.last_remove_ms()
    b.finish()
    for _ in range(2):
        render()
    eng.wait()
    res["remove"] = dict(instances_ms=round(1e3 * (t1 - t0), 2), builder_ms=round(1e3 * (t2 - t1), 2), call_ms=round(1e3 * (t3 - t2), 3),
                         call_to_frame_end_ms=round(1e3 * (t4 - t2), 2), triangles_removed=tris, launches=launches, runs_per_plane=runs, path=path, bytes_moved=moved,
                         compaction_launch_ms=round(launch_ms, 4), compaction_gb_s=round(2 * moved / max(launch_ms, 1e-6) / 1e6, 1),
                         mesh_level_laid_out_again=int(eng.stats().scene_mesh_builds) - builds)
    res["held_after_remove_mb"] = held_mb()   # (the old allocation is still held: it is freed where the host next waits for every stream)
    eng.read_mesh_nodes()
    res["held_after_remove_and_wait_mb"] = held_mb()
    t5 = time.perf_counter()
    eng.load_scene(b, F.TREE_SAH)
    t6 = time.perf_counter()
    render()
    eng.wait()
    t7 = time.perf_counter()
    res["load"] = dict(call_ms=round(1e3 * (t6 - t5), 2), call_to_frame_end_ms=round(1e3 * (t7 - t5), 2))
    res["held_after_load_mb"] = held_mb()
    # (hk_load_scene lays the scene out at its first use: the frame's end is where both routes have done their work)
    res["load_over_remove_to_frame_end"] = round(res["load"]["call_to_frame_end_ms"] / max(res["remove"]["call_to_frame_end_ms"], 1e-3), 1)
    copy_gb_s, _ = eng.measure_hbm()
    res["measured_hbm_copy_gb_s"] = round(copy_gb_s, 1)
    res["compaction_over_copy_rate"] = round(res["remove"]["compaction_gb_s"] / max(copy_gb_s, 1e-6), 3)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main(argv):
    if len(argv) >= 3 and argv[0] == "--child":
        return child(argv[1], argv[2])
    out_path = os.path.join(ROOT, "profiles", "remove_mesh_probe.json")
    if "--out" in argv:
        k = argv.index("--out")
        out_path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    results = []
    for name in argv or SCENES:
        for shape in SHAPES:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, shape], capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout + r.stderr, file=sys.stderr)
                raise SystemExit(f"{name} / {shape}: the probe failed")
            results.append(json.loads(line[-1][7:]))
            print(json.dumps(results[-1]), flush=True)
    doc = {"what": "meshes leaving a loaded scene, ms: hk_remove_meshes (one mesh / every tenth mesh; host time of the call, call to the end of the next frame, the "
                   "compaction launch between two HIP events and its read + written bytes over that time) against hk_load_scene of the remaining builder in the same "
                   "process, hk_measure_hbm's copy rate of the same process, and the device memory the process holds (one run each, one process per entry; 960x540, "
                   "one bounce)", "entries": results}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
