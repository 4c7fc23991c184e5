#!/usr/bin/env python3
"""A mesh whose arrays live in device memory arriving in a loaded, rendering scene: hk_add_meshes_device against the host route, in the
scenes of tools/add_mesh_probe.py - one process per (scene, added size).  In each process two contexts load the same scene (each from a
builder of its own) and render; then meshes of the same size arrive, one warm-up arrival and five measured ones per path, alternately:
  host    tensor.cpu() of the four arrays (behind a wait for their producer) + add_mesh(build_tree=False) + finish + hk_add_meshes
  device  declare_mesh + finish + hk_add_meshes_device naming the tensors
Per arrival: the host time of every step, and the time from the first step to the end of the next frame (the steps, the instance update
that gives the mesh its instance, one frame).  For the device path also hk_debug_last_add_source_times - the assembling launch between
two HIP events with the bytes it moves (per triangle 12 B of indices, 36 B gathered, 48 B stored; per vertex 32 B read, 32 B stored)
against hk_measure_hbm's copy rate of the same process, the wait with the read-back, the builder's store.  Medians of the five; the
warm-up arrival (which moves the scene to a roomier allocation) is reported apart.  One run per entry.  Not part of bench.py.
Usage: python tools/mesh_source_probe.py [--out FILE] [--sizes N,N,...] [scene ...]      scenes: mesh_1e5 mesh_1e6 many_meshes"""
import json
import os
import statistics
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

SCENES = ("mesh_1e5",)
ADDED = (10_000, 100_000, 1_000_000)
MEASURED = 5


def child(name, triangles):
    import torch

    runs = {}
    for path in ("host", "device"):
        eng = hk.Engine(device=0, flags=0)
        eng.upload_noise()
        eng.resize(960, 540, 1.0)
        with Meter(deferred=True):
            b, textures, sun, cam = MAKERS[name]()
        eng.load_scene(b, F.TREE_SAH, textures)
        eng.set_debug_option(F.DEBUG_OPT_ADD_SOURCE_TIMES, 1)
        runs[path] = dict(eng=eng, b=b, frame=0, arrivals=[])
    lights, s = hk.lights_uniform(directional=sun), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()

    def render(r):
        r["frame"] += 1
        r["eng"].frame_render(hk.frame_uniform(s, r["frame"]), view, pview, lights, s.to_c())

    for r in runs.values():
        for _ in range(4):
            render(r)
        r["eng"].wait()
    p, n, uv, idx = S.large_cloth(triangles)
    n_tris, n_verts = len(idx) // 3, len(p)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    tensors = dict(positions=dev(p), normals=dev(n), uvs=dev(uv), indices=dev(idx.view("int32")))
    ms = lambda a, b: round(1e3 * (b - a), 3)
    for k in range(MEASURED + 1):
        tensors["positions"] += 0.01   # (a producer: every arrival's positions are made on the device right before it)
        for path, r in runs.items():
            eng, b = r["eng"], r["b"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if path == "host":
                arrays = [tensors[key].cpu().numpy() for key in ("positions", "normals", "uvs", "indices")]
                t1 = time.perf_counter()
                mesh = b.add_mesh(arrays[0], arrays[1], arrays[2], arrays[3].view("uint32"), build_tree=False)
                t2 = time.perf_counter()
                b.finish()
                t3 = time.perf_counter()
                eng.add_meshes(b, F.TREE_SAH)
                t4 = time.perf_counter()
                steps = dict(tensor_cpu_ms=ms(t0, t1), add_mesh_deferred_ms=ms(t1, t2), finish_ms=ms(t2, t3), add_meshes_ms=ms(t3, t4))
            else:
                mesh = b.declare_mesh(n_verts, len(idx))
                t1 = time.perf_counter()
                b.finish()
                t2 = time.perf_counter()
                eng.add_meshes(b, F.TREE_SAH, sources={mesh: tensors})
                t4 = time.perf_counter()
                kernel, readback, store = eng.last_add_source_times()
                steps = dict(declare_mesh_ms=ms(t0, t1), finish_ms=ms(t1, t2), add_meshes_device_ms=ms(t2, t4), assemble_kernel_ms=round(kernel, 4),
                             wait_and_readback_ms=round(readback, 3), builder_store_ms=round(store, 3), staged_record_bytes=eng.last_add_sources()[3])
            steps["relocated"] = eng.last_add()[4]
            b.add_instance(mesh, 0, S._trs((0.3 * k, 2.5, 0.0), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)))
            eng.update_instances_on_device(b, F.TREE_SAH)
            render(r)
            eng.wait()
            steps["steps_ms"] = ms(t0, t4)
            steps["to_frame_end_ms"] = ms(t0, time.perf_counter())
            r["arrivals"].append(steps)
            for _ in range(2):
                render(r)
            eng.wait()
    copy_gbs, _ = runs["device"]["eng"].measure_hbm()
    moved = n_tris * (12 + 36 + 48) + n_verts * (32 + 32)
    res = {"scene": name, "added_triangles": n_tris, "added_vertices": n_verts, "hbm_copy_gb_s": round(copy_gbs, 1), "assemble_bytes_moved": moved}
    for path, r in runs.items():
        first, rest = r["arrivals"][0], r["arrivals"][1:]
        res[path] = {key: statistics.median(a[key] for a in rest) for key in rest[0]}
        res[path]["relocations_among_the_measured"] = sum(a["relocated"] for a in rest)
        res[path]["warm_up_arrival"] = first
        r["eng"].close()
    kernel_ms = res["device"]["assemble_kernel_ms"]
    res["assemble_gb_s"] = round(moved / max(kernel_ms, 1e-6) / 1e6, 1)
    res["assemble_fraction_of_copy_rate"] = round(res["assemble_gb_s"] / copy_gbs, 3)
    res["device_over_host_steps"] = round(res["device"]["steps_ms"] / res["host"]["steps_ms"], 3)
    res["device_over_host_to_frame_end"] = round(res["device"]["to_frame_end_ms"] / res["host"]["to_frame_end_ms"], 3)
    print("RESULT " + json.dumps(res), flush=True)


def main(argv):
    if len(argv) >= 3 and argv[0] == "--child":
        return child(argv[1], int(argv[2]))
    out_path = os.path.join(ROOT, "profiles", "mesh_source_probe.json")
    sizes = ADDED
    for flag in ("--out", "--sizes"):
        if flag in argv:
            k = argv.index(flag)
            if flag == "--out":
                out_path = argv[k + 1]
            else:
                sizes = tuple(int(v) for v in argv[k + 1].split(","))
            argv = argv[:k] + argv[k + 2:]
    results = []
    for name in argv or SCENES:
        for triangles in sizes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(triangles)], capture_output=True, text=True, timeout=420)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout + r.stderr, file=sys.stderr)
                raise SystemExit(f"{name} + {triangles}: the probe failed")
            results.append(json.loads(line[-1][7:]))
            print(json.dumps(results[-1]), flush=True)
    doc = {"what": "one mesh whose arrays are torch tensors on the device arriving in a loaded, rendering scene, ms: the host route (tensor.cpu() + add_mesh deferred + finish + "
                   "hk_add_meshes) against declare_mesh + finish + hk_add_meshes_device, both in one process, each on a context of its own, taken alternately; medians of "
                   f"{MEASURED} arrivals behind one warm-up arrival (ONE run, one process per entry; 960x540, one bounce); assemble_gb_s: the bytes the assembling launch moves "
                   "over its time between two HIP events, next to hk_measure_hbm's copy rate of the same process", "entries": results}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
