#!/usr/bin/env python3
"""Instance poses that live in a torch tensor on the device, handed to the renderer two ways - each on a context of its own, over the same
scene (2 000 and 20 000 instances; 15 % and 100 % of them moving per frame), in one process:
 (a) the host path: tensor.cpu(), hk_scene_builder_set_instance_transform once per instance (the host does not know who moved: the refit's
     own diff finds out), hk_refit_scene_instances;
 (b) hk_set_instance_transforms_device with all poses (ids NULL): the tensor is read where it lies, who moved is decided on the device.
The poses are produced by torch ops on a stream of the probe's, behind a matrix product that takes a while - what a simulation step looks
like to the renderer - and neither path is told when they are ready: (a) waits for them inside tensor.cpu(), (b) orders its stream by an event.
Per case, medians over the repeats: the host time of each path up to the return of its last call (for (a) also its three parts; the
per-instance calls are made from Python through ctypes, about a microsecond each), and the time from the start of the path to the end
of the next frame (960 x 540, one bounce; host clock around a wait for the device).
Usage: python tools/pose_source_probe.py [--out FILE] [--repeats N] [INSTANCES ...]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import Camera, look_at_transform
from bevy_hikari_amd.scenes import synthetic_large


def probe(n_instances, fraction, repeats=5):
    import torch

    dev = torch.device("cuda", 0)
    sim = torch.cuda.Stream(dev)           # the producer
    cam = Camera(look_at_transform((48.0, 33.0, 60.0), (0.0, 0.6, 0.0)), 960, 540)
    s = hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    paths = {}
    for name in ("a", "b"):
        scene, sun = synthetic_large(0x5EED0004, 20, 16, 32, n_instances, 50, 8, 40.0)
        eng = hk.Engine(device=0, flags=0)
        eng.upload_noise()
        eng.upload_scene(scene)
        eng.resize(960, 540, 1.0)
        paths[name] = dict(eng=eng, builder=scene.builder, lights=hk.lights_uniform(directional=sun), frame=0)
    rest = np.array([np.ctypeslib.as_array(i.model).copy() for i in scene.instances], dtype=np.float32)
    n = len(rest)
    rng = np.random.default_rng(11)
    movers = torch.from_numpy(np.sort(rng.choice(n, size=max(1, int(round(fraction * n))), replace=False))).to(dev)
    rest_t = torch.from_numpy(rest).to(dev)
    busy = torch.randn((1024, 1024), device=dev)
    torch.cuda.synchronize()

    def frame(p):
        p["frame"] += 1
        p["eng"].frame_render(hk.frame_uniform(s, p["frame"]), view, pview, p["lights"], s.to_c())

    def produce(k):   # the simulation's stand-in, enqueued and not waited for: a step of work, then the movers' translations
        with torch.cuda.stream(sim):
            x = busy
            for _ in range(4):
                x = torch.mm(x, x) * 1e-3
            poses = rest_t.clone()
            poses[movers, 12] += 0.02 * k
            poses[movers, 13] += 0.01 * k
        return poses

    set_transform = F.api().raw("scene_builder_set_instance_transform")
    fp = C.POINTER(F.f32)

    def path_a(p, poses):
        t0 = time.perf_counter()
        with torch.cuda.stream(sim):
            host = poses.cpu().numpy()        # waits for the producer
        t1 = time.perf_counter()
        base, h = host.ctypes.data, p["builder"].h
        for i in range(n):
            set_transform(h, i, C.cast(base + 64 * i, fp))
        t2 = time.perf_counter()
        moved = p["eng"].refit_instances(p["builder"])
        t3 = time.perf_counter()
        assert moved == len(movers), (moved, len(movers))
        return t0, (t1 - t0, t2 - t1, t3 - t2), t3

    def path_b(p, poses):
        t0 = time.perf_counter()
        p["eng"].set_instance_transforms(p["builder"], poses, producer_stream=sim)
        return t0, (), time.perf_counter()

    rows = {"a": [], "b": []}
    for r in range(repeats + 2):   # (the first two rounds warm both paths: refit planes, the mesh-box plane, staging blocks)
        for name, path in (("a", path_a), ("b", path_b)):
            p = paths[name]
            frame(p)
            p["eng"].wait()
            torch.cuda.synchronize()
            poses = produce(r + 1)
            t0, parts, t1 = path(p, poses)
            frame(p)
            p["eng"].wait()
            t2 = time.perf_counter()
            if r >= 2:
                rows[name].append((1e3 * (t1 - t0), 1e3 * (t2 - t0)) + tuple(1e3 * q for q in parts))
    launches, copied = paths["b"]["eng"].last_pose()
    sim.synchronize()
    t0 = time.perf_counter()
    for _ in range(8):
        frame(paths["b"])
    paths["b"]["eng"].wait()
    frame_ms = 1e3 * (time.perf_counter() - t0) / 8
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(sim):
        e0.record(sim)
        produce(99)
        e1.record(sim)
    e1.synchronize()
    med = lambda v: round(float(np.median(v)), 4)
    col = lambda name, k: med([row[k] for row in rows[name]])
    out = {"instances": n, "moving": int(len(movers)), "frame_alone_ms": round(frame_ms, 3), "producer_step_ms": round(e0.elapsed_time(e1), 3),
           "host_path_call_ms": col("a", 0), "host_path_to_frame_end_ms": col("a", 1),
           "host_path_tensor_cpu_ms": col("a", 2), "host_path_set_transforms_ms": col("a", 3), "host_path_refit_call_ms": col("a", 4),
           "device_path_call_ms": col("b", 0), "device_path_to_frame_end_ms": col("b", 1), "device_path_launches": launches,
           "device_path_warm_call_copied_mesh_boxes": copied,
           "device_path_call_ms_range": [round(min(r[0] for r in rows["b"]), 4), round(max(r[0] for r in rows["b"]), 4)],
           "host_path_call_ms_range": [round(min(r[0] for r in rows["a"]), 4), round(max(r[0] for r in rows["a"]), 4)]}
    for p in paths.values():
        p["eng"].wait()
        p["eng"].close()
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
    for n in [int(a) for a in args] or [2_000, 20_000]:
        for fraction in (0.15, 1.0):
            row = probe(n, fraction, repeats)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if path:
        with open(path, "w") as fh:
            json.dump({"probe": "tools/pose_source_probe.py", "rows": rows}, fh, indent=1)
