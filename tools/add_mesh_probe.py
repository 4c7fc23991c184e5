#!/usr/bin/env python3
"""Meshes added to a loaded scene: hk_add_meshes against hk_load_scene of the whole builder (the only route before it), in the scenes of
tools/load_probe.py - one mesh of 10^5 / 10^6 triangles, 2 000 meshes of 750 - one process per (scene, added size).  In each process the
scene is loaded with device-built trees and rendered, then three deferred meshes of the same size arrive one after the other:
  first   hk_add_meshes; the capacities of a fresh load are exact, so this add moves the scene to a roomier allocation
  second  hk_add_meshes; fits the room the first one left
  load    hk_load_scene of the whole builder, in the same process state (the baseline: the full host layout)
Per arrival: the builder's finish, the host time of the call (and where it went: hk_debug_last_add_times), and the time from the call to the end of the next frame (the call, the
instance update that gives the mesh its instance - hk_update_scene_instances, or nothing more for the load - and one frame).  One run per
entry.  Not part of bench.py.
Usage: python tools/add_mesh_probe.py [--out FILE] [scene ...]      scenes: mesh_1e5 mesh_1e6 many_meshes"""
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
ADDED = (1_000, 10_000)


def child(name, triangles):
    eng = hk.Engine(device=0, flags=0)
    eng.upload_noise()
    eng.resize(960, 540, 1.0)
    with Meter(deferred=True):
        b, textures, sun, cam = MAKERS[name]()
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
    p, n, uv, idx = S.large_cloth(triangles)
    res = {"scene": name, "scene_mesh_nodes": nodes, "orderings": orderings, "added_triangles": len(idx) // 3}
    for k, arrival in enumerate(("first", "second", "load")):
        t0 = time.perf_counter()
        mesh = b.add_mesh(p + 0.01 * k, n, uv, idx, build_tree=False)
        if arrival == "load":
            b.add_instance(mesh, 0, S._trs((0.3 * k, 2.5, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)))
        b.finish()
        t1 = time.perf_counter()
        if arrival == "load":
            eng.load_scene(b, F.TREE_SAH)
            t2 = time.perf_counter()
            what = dict(zip(("device_meshes", "device_triangles", "build_launches", "host_meshes"), eng.last_load()))
        else:
            eng.add_meshes(b, F.TREE_SAH)
            t2 = time.perf_counter()
            what = dict(zip(("device_meshes", "device_triangles", "build_launches", "host_meshes", "relocated"), eng.last_add()))
            what.update(zip(("relocation_alloc_ms", "relocation_copy_and_switch_ms", "mirrors_ms", "stage_build_readback_ms"), (round(v, 3) for v in eng.last_add_times())))
            b.add_instance(mesh, 0, S._trs((0.3 * k, 2.5, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)))
            eng.update_instances_on_device(b, F.TREE_SAH)
        render()
        eng.wait()
        t3 = time.perf_counter()
        res[arrival] = dict(builder_ms=round(1e3 * (t1 - t0), 2), call_ms=round(1e3 * (t2 - t1), 2), call_to_frame_end_ms=round(1e3 * (t3 - t1), 2), **what)
        for _ in range(2):
            render()
        eng.wait()
    res["relocation_ms"] = round(res["first"]["call_ms"] - res["second"]["call_ms"], 2)
    res["load_over_add_call"] = round(res["load"]["call_ms"] / max(res["second"]["call_ms"], 1e-3), 1)
    res["scene_mesh_builds"] = int(eng.stats().scene_mesh_builds)
    eng.close()
    print("RESULT " + json.dumps(res), flush=True)


def main(argv):
    if len(argv) >= 3 and argv[0] == "--child":
        return child(argv[1], int(argv[2]))
    out_path = os.path.join(ROOT, "profiles", "add_mesh_probe.json")
    if "--out" in argv:
        k = argv.index("--out")
        out_path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    results = []
    for name in argv or SCENES:
        for triangles in ADDED:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(triangles)], capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout + r.stderr, file=sys.stderr)
                raise SystemExit(f"{name} + {triangles}: the probe failed")
            results.append(json.loads(line[-1][7:]))
            print(json.dumps(results[-1]), flush=True)
    doc = {"what": "one deferred mesh arriving in a loaded scene, ms: hk_add_meshes (first: with the one move to a roomier allocation; second: into that room) "
                   "against hk_load_scene of the whole builder in the same process (one run each, one process per entry; 960x540, one bounce)", "entries": results}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
