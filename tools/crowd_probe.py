#!/usr/bin/env python3
"""A crowd of skinned meshes per frame: the same poses through a loop of single calls (hk_skin_mesh, one mesh each) and through one
batch (hk_deform_meshes), in one process on one context - K = 16, 128, 512 meshes of 500 and 5 000 triangles in a scene beyond the LDS
copy (eight orderings, wide records).  Per configuration, medians over the repeats: the host time of the calls (the C entry points with
their arguments prepared beforehand), the time from the first call to the end of the next frame (960 x 540, one bounce), and the launch
counts - what the batch enqueued, the flush and the wide-record derivation of the frame that followed (hk_debug_last_deform); a single
hk_skin_mesh enqueues 3 memsets and 5 kernels.
Usage: python tools/crowd_probe.py [--out FILE] [--repeats N] [K:TRIANGLES ...]"""
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
from bevy_hikari_amd.plugin import Camera, deform_items, look_at_transform

SINGLE_CALL_ENQUEUES = 8   # hk_skin_mesh: 2 memsets of the box, the palette copy, skin, triangles, the counters' memset, boxes, emit


def probe(k_meshes, triangles, repeats=7):
    scene, sun, meshes = S.crowd_scene("yard", [triangles] * k_meshes, skinned=lambda k: True)
    eng = hk.Engine(device=0, flags=0)
    eng.upload_noise()
    eng.upload_scene(scene)
    eng.resize(960, 540, 1.0)
    for m in meshes.values():
        eng.set_mesh_skin(m["index"], m["rest"], m["normals"], m["joints"], m["weights"])
    cam = Camera(look_at_transform((6.4, 4.4, 8.0), (0.0, 0.6, 0.0)), 960, 540)
    lights, s = hk.lights_uniform(directional=sun), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    frame_no = [0]

    def frame():
        frame_no[0] += 1
        eng.frame_render(hk.frame_uniform(s, frame_no[0]), view, pview, lights, s.to_c())

    skin, batch = eng.api.raw("skin_mesh"), eng.api.raw("deform_meshes")
    fp = C.POINTER(F.f32)

    def single(items):
        args = [(C.byref(it[1]), it[2].ctypes.data_as(fp), len(it[2])) for it in items]
        t0 = time.perf_counter()
        for mesh, joints, n in args:
            if skin(eng.ctx, mesh, joints, n) != F.HK_OK:
                raise RuntimeError(eng.api.last_error())
        return t0, time.perf_counter()

    def batched(items):
        table, keep = deform_items(items)
        t0 = time.perf_counter()
        if batch(eng.ctx, table, len(items)) != F.HK_OK:
            raise RuntimeError(eng.api.last_error())
        return t0, time.perf_counter()

    rows = {"single": [], "batch": []}
    counts = {}
    for r in range(repeats + 2):   # (the first two rounds warm both paths: refit planes, staging blocks, palettes)
        for name, call in (("single", single), ("batch", batched)):
            items = [(m["kind"], m["index"], np.ascontiguousarray(m["pose"](2 * r + (name == "batch"))[0], np.float32)) for m in meshes.values()]
            frame()
            eng.wait()
            t0, t1 = call(items)
            frame()
            eng.wait()
            t2 = time.perf_counter()
            if r >= 2:
                rows[name].append((1e3 * (t1 - t0), 1e3 * (t2 - t0)))
            counts[name] = eng.last_deform()
    t0 = time.perf_counter()
    for _ in range(8):
        frame()
    eng.wait()
    frame_ms = 1e3 * (time.perf_counter() - t0) / 8
    med = lambda name, k: round(float(np.median([row[k] for row in rows[name]])), 4)
    out = {"meshes": k_meshes, "triangles_per_mesh": triangles, "vertices_per_mesh": triangles + 2, "instances": len(scene.instances),
           "frame_alone_ms": round(frame_ms, 3),
           "single_calls_host_ms": med("single", 0), "batch_call_host_ms": med("batch", 0),
           "single_first_call_to_frame_end_ms": med("single", 1), "batch_first_call_to_frame_end_ms": med("batch", 1),
           "single_call_enqueues": SINGLE_CALL_ENQUEUES * k_meshes, "batch_call_enqueues": counts["batch"][3],
           "single_flush_launches": counts["single"][4], "batch_flush_launches": counts["batch"][4],
           "single_wide_launches": counts["single"][5], "batch_wide_launches": counts["batch"][5]}
    eng.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    path, repeats = None, 7
    while args[:1] in (["--out"], ["--repeats"]):
        if args[0] == "--out":
            path = args[1]
        else:
            repeats = int(args[1])
        args = args[2:]
    configs = [tuple(int(v) for v in a.split(":")) for a in args] or [(16, 500), (128, 500), (512, 500), (16, 5000), (128, 5000), (512, 5000)]
    rows = []
    for k, t in configs:
        row = probe(k, t, repeats)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if path:
        with open(path, "w") as fh:
            json.dump({"probe": "tools/crowd_probe.py", "rows": rows}, fh, indent=1)
