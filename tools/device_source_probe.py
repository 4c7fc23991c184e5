#!/usr/bin/env python3
"""One grid mesh of 10^4, 10^5 and 10^6 vertices whose positions live in a torch tensor on the device, deformed two ways on one context:
 (a) the host path: tensor.cpu(), the normals from the builder's twin on the host (hk_scene_builder_set_mesh_vertices +
     hk_scene_builder_recompute_mesh_normals + finish), then hk_deform_meshes with positions and normals from host memory;
 (b) hk_deform_meshes_device with HK_DEFORM_RECOMPUTE_NORMALS: the tensor is read where it lies, the normals are recomputed on the device.
Per size, medians over the repeats: the host time of each path up to the return of the deformation call (for (a) also its three parts),
the time from the start of the path to the end of the next frame (960 x 540, one bounce; host clock around a wait for the device), and
- from HIP events on the context's stream, which the probe owns for that - the device time of batch (b) with and without the flag; their
difference is the normals launch (with the face vectors the triangle launch writes for it); the ranges beside them show the spread.
Usage: python tools/device_source_probe.py [--out FILE] [--repeats N] [VERTICES ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import Camera, deform_items, deform_items_device, look_at_transform


def grid_scene(side):
    scene, sun = S.synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    p, n, uv, idx = S.cloth_grid(side - 1, side - 1, size=3.0)
    mesh = b.add_mesh(p, n, uv, idx)
    b.add_instance(mesh, b.add_material(S.standard_material((0.3, 0.6, 0.8, 1.0), (0, 0, 0), 0.6, 0.0, 0.5)), S._trs((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    scene = b.finish()
    return scene, sun, b, mesh, p


def probe(vertices, repeats=5):
    import torch

    side = max(2, int(round(vertices ** 0.5)))
    scene, sun, builder, mesh_id, rest = grid_scene(side)
    index = builder.mesh_index(mesh_id)
    _scene, _sun, mirror, mirror_id, _rest = grid_scene(side)   # the host's mirror: a builder of its own
    nv = len(rest)
    dev = torch.device("cuda", 0)
    eng = hk.Engine(device=0, flags=0)
    stream = torch.cuda.Stream(dev)
    eng.set_stream(stream.cuda_stream)
    eng.upload_noise()
    eng.upload_scene(scene)
    eng.resize(960, 540, 1.0)
    cam = Camera(look_at_transform((4.0, 3.5, 5.0), (0.0, 0.8, 0.0)), 960, 540)
    lights, s = hk.lights_uniform(directional=sun), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    frame_no = [0]

    def frame():
        frame_no[0] += 1
        eng.frame_render(hk.frame_uniform(s, frame_no[0]), view, pview, lights, s.to_c())

    rest_t = torch.from_numpy(rest).to(dev)

    def produce(k):   # the simulation's stand-in: positions on the device, a wave that moves with k
        with torch.cuda.stream(stream):
            q = rest_t.clone()
            q[:, 1] = 0.2 * torch.sin(3.0 * rest_t[:, 0] + 0.3 * k) * torch.cos(2.0 * rest_t[:, 2])
        stream.synchronize()
        return q

    host_call, device_call = eng.api.raw("deform_meshes"), eng.api.raw("deform_meshes_device")

    def path_a(q):
        t0 = time.perf_counter()
        pos = q.cpu().numpy()
        t1 = time.perf_counter()
        mirror.set_mesh_vertices(mirror_id, pos)
        mirror.recompute_mesh_normals(mirror_id)
        mirrored = mirror.finish()
        mi = mirror.mesh_index(mirror_id)
        nrm = np.frombuffer(bytes(mirrored.vertices), np.float32).reshape(-1, 8)[mi.vertex:mi.vertex + nv, 4:7]
        table, keep = deform_items([("vertices", index, pos, nrm)])
        t2 = time.perf_counter()
        if host_call(eng.ctx, table, 1) != F.HK_OK:
            raise RuntimeError(eng.api.last_error())
        t3 = time.perf_counter()
        return t0, (t1 - t0, t2 - t1, t3 - t2), t3

    def path_b(q, flags=F.DEFORM_RECOMPUTE_NORMALS):
        t0 = time.perf_counter()
        table, keep = deform_items_device([("vertices", index, q, None, dict(recompute_normals=bool(flags)))], 0)
        if device_call(eng.ctx, table, 1, None) != F.HK_OK:   # (the tensor is complete and the context runs on the probe's stream: nothing to order)
            raise RuntimeError(eng.api.last_error())
        return t0, (), time.perf_counter()

    rows = {"a": [], "b": []}
    for r in range(repeats + 2):   # (the first two rounds warm both paths: refit planes, the corner list, staging blocks)
        for name, path in (("a", path_a), ("b", path_b)):
            q = produce(2 * r + (name == "b"))
            frame()
            eng.wait()
            t0, parts, t1 = path(q)
            frame()
            eng.wait()
            t2 = time.perf_counter()
            if r >= 2:
                rows[name].append((1e3 * (t1 - t0), 1e3 * (t2 - t0)) + tuple(1e3 * p for p in parts))
    launches = eng.last_deform()[3]
    # the device time of batch (b) alone, flagged and not, alternating, from events on the context's stream
    device_ms = {0: [], F.DEFORM_RECOMPUTE_NORMALS: []}
    for r in range(2 * repeats + 2):
        for flags in (F.DEFORM_RECOMPUTE_NORMALS, 0):
            q = produce(r)
            eng.wait()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            path_b(q, flags)
            e1.record(stream)
            e1.synchronize()
            if r >= 2:
                device_ms[flags].append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    for _ in range(8):
        frame()
    eng.wait()
    frame_ms = 1e3 * (time.perf_counter() - t0) / 8
    med = lambda v: round(float(np.median(v)), 4)
    col = lambda name, k: med([row[k] for row in rows[name]])
    flagged, plain = med(device_ms[F.DEFORM_RECOMPUTE_NORMALS]), med(device_ms[0])
    out = {"vertices": nv, "triangles": 2 * (side - 1) ** 2, "frame_alone_ms": round(frame_ms, 3),
           "host_path_call_ms": col("a", 0), "host_path_to_frame_end_ms": col("a", 1),
           "host_path_tensor_cpu_ms": col("a", 2), "host_path_builder_normals_ms": col("a", 3), "host_path_deform_call_ms": col("a", 4),
           "device_path_call_ms": col("b", 0), "device_path_to_frame_end_ms": col("b", 1), "device_path_launches": launches,
           "device_batch_flagged_ms": flagged, "device_batch_unflagged_ms": plain, "normals_launch_ms": round(flagged - plain, 4),
           "device_batch_flagged_ms_range": [round(min(device_ms[F.DEFORM_RECOMPUTE_NORMALS]), 4), round(max(device_ms[F.DEFORM_RECOMPUTE_NORMALS]), 4)],
           "device_batch_unflagged_ms_range": [round(min(device_ms[0]), 4), round(max(device_ms[0]), 4)]}
    eng.wait()
    eng.set_stream(0)
    eng.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    path, repeats = None, 5
    while args[:1] in (["--out"], ["--repeats"]):
        if args[0] == "--out":
            path = args[1]
        else:
            repeats = int(args[1])
        args = args[2:]
    rows = []
    for n in [int(a) for a in args] or [10_000, 100_000, 1_000_000]:
        row = probe(n, repeats)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if path:
        with open(path, "w") as fh:
            json.dump({"probe": "tools/device_source_probe.py", "rows": rows}, fh, indent=1)
