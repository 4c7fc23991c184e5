#!/usr/bin/env python3
"""A texture that lives in a torch tensor on the device - the base colour of the textured yard's ground, 1024^2 and 4096^2, as a uint8 HWC
tensor and as a float32 CHW tensor (4 channels: 256 MB at 4096^2) - handed to the renderer two ways, each on a context of its own, in one
process:
 (a) the host path: tensor.cpu(), for float data the quantisation in numpy (clip, x 255 + 0.5, to bytes, planes to pixels), then
     hk_update_texture, which copies the bytes once more into pinned staging;
 (b) Engine.update_textures (hk_update_textures_device): the tensor is read where it lies, converted by one kernel.
The tensor is produced by torch ops on a stream of the probe's, behind a matrix product that takes a while, and neither path is told when
it is ready: (a) waits for it inside tensor.cpu(), (b) orders its stream by an event.  Per case, medians over the repeats: the host time
of each path up to the return of its last call (for (a) also its parts) and the time from the start of the path to the end of the next
frame (960 x 540, one bounce; host clock around a wait for the device).
Then a batch: 64 textures of 256^2 (uint8 HWC, one tensor) through tensor.cpu() + 64 hk_update_texture calls - one launch each - and
through ONE device call, its launches read from hk_debug_last_texture_update.
Usage: python tools/texture_source_probe.py [--out FILE] [--repeats N] [SIZE ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.scenes import synthetic_camera, synthetic_scene

GROUND = 0   # scenes._test_textures: the checker, the ground's base colour


def contexts(textures_of):
    """two engines over the textured yard whose texture list is textures_of(the yard's own)"""
    paths = {}
    for name in ("a", "b"):
        scene, sun = synthetic_scene(textured=True)
        scene.textures = textures_of(list(scene.textures))
        eng = hk.Engine(device=0, flags=0)
        eng.upload_noise()
        eng.upload_scene(scene)
        eng.resize(960, 540, 1.0)
        paths[name] = dict(eng=eng, lights=hk.lights_uniform(directional=sun), frame=0, sampler={k: v for k, v in scene.textures[GROUND].items() if k != "rgba"})
    return paths


def quantise(x):
    """float planes [4][h][w] -> bytes [h][w][4]: what a host does today before hk_update_texture"""
    return np.ascontiguousarray(np.moveaxis((np.clip(np.nan_to_num(x), 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8), 0, 2))


def probe(size, kind, repeats=5):
    import torch

    dev = torch.device("cuda", 0)
    sim = torch.cuda.Stream(dev)
    cam = synthetic_camera(960, 540)
    s = hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    rng = np.random.default_rng(size)
    first = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
    paths = contexts(lambda t: [dict(t[GROUND], rgba=first)] + t[1:])
    base = torch.from_numpy(first).to(dev) if kind == "uint8_hwc" else torch.from_numpy(np.moveaxis(first, 2, 0).astype(np.float32) / np.float32(255.0)).to(dev)
    layout = "hwc" if kind == "uint8_hwc" else "chw"
    busy = torch.randn((1024, 1024), device=dev)
    torch.cuda.synchronize()

    def frame(p):
        p["frame"] += 1
        p["eng"].frame_render(hk.frame_uniform(s, p["frame"]), view, pview, p["lights"], s.to_c())

    def produce(k):   # the producer's stand-in, enqueued and not waited for: a step of work, then the new texels
        with torch.cuda.stream(sim):
            x = busy
            for _ in range(4):
                x = torch.mm(x, x) * 1e-3
            return base + k if kind == "uint8_hwc" else base * (1.0 - 0.01 * k)

    def path_a(p, tensor):
        t0 = time.perf_counter()
        with torch.cuda.stream(sim):
            host = tensor.cpu().numpy()        # waits for the producer
        t1 = time.perf_counter()
        rgba = host if kind == "uint8_hwc" else quantise(host)
        t2 = time.perf_counter()
        p["eng"].update_texture(GROUND, dict(p["sampler"], rgba=rgba))
        t3 = time.perf_counter()
        return t0, (t1 - t0, t2 - t1, t3 - t2), t3

    def path_b(p, tensor):
        t0 = time.perf_counter()
        p["eng"].update_textures([dict(index=GROUND, tensor=tensor, layout=layout)], producer_stream=sim)
        return t0, (), time.perf_counter()

    rows = {"a": [], "b": []}
    for r in range(repeats + 2):   # (the first two rounds warm both paths: staging blocks, the allocator's pinned and device blocks)
        for name, path in (("a", path_a), ("b", path_b)):
            p = paths[name]
            frame(p)
            p["eng"].wait()
            torch.cuda.synchronize()
            tensor = produce(r + 1)
            t0, parts, t1 = path(p, tensor)
            frame(p)
            p["eng"].wait()
            t2 = time.perf_counter()
            if r >= 2:
                rows[name].append((1e3 * (t1 - t0), 1e3 * (t2 - t0)) + tuple(1e3 * q for q in parts))
    items, launches, texels = paths["b"]["eng"].last_texture_update()
    sim.synchronize()
    same = bool(np.array_equal(paths["a"]["eng"].read_texture(GROUND), paths["b"]["eng"].read_texture(GROUND)))
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
    # the conversion by itself, on the device's clock: both sides idle, events on the producer stream around the call - the stream waits
    # for the kernel that reads the tensor, so the span is the kernel plus the two event hand-overs
    kernel = []
    tensor = produce(100)
    for _ in range(repeats + 2):
        paths["b"]["eng"].wait()
        torch.cuda.synchronize()
        k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(sim):
            k0.record(sim)
            paths["b"]["eng"].update_textures([dict(index=GROUND, tensor=tensor, layout=layout)], producer_stream=sim)
            k1.record(sim)
        k1.synchronize()
        kernel.append(k0.elapsed_time(k1))
    kernel = kernel[2:]
    med = lambda v: round(float(np.median(v)), 4)
    col = lambda name, k: med([row[k] for row in rows[name]])
    out = {"texture": f"{size} x {size}", "source": kind, "source_bytes": int(base.numel() * base.element_size()), "frame_alone_ms": round(frame_ms, 3),
           "producer_step_ms": round(e0.elapsed_time(e1), 3),
           "host_path_call_ms": col("a", 0), "host_path_to_frame_end_ms": col("a", 1),
           "host_path_tensor_cpu_ms": col("a", 2), "host_path_quantise_ms": col("a", 3), "host_path_update_texture_ms": col("a", 4),
           "device_path_call_ms": col("b", 0), "device_path_to_frame_end_ms": col("b", 1), "device_path_launches": launches, "device_path_texels": texels,
           "device_path_kernel_span_ms": med(kernel), "device_path_kernel_span_ms_range": [round(min(kernel), 4), round(max(kernel), 4)],
           "device_path_call_ms_range": [round(min(r[0] for r in rows["b"]), 4), round(max(r[0] for r in rows["b"]), 4)],
           "host_path_call_ms_range": [round(min(r[0] for r in rows["a"]), 4), round(max(r[0] for r in rows["a"]), 4)],
           "both_paths_left_the_same_texels": same}
    for p in paths.values():
        p["eng"].wait()
        p["eng"].close()
    return out


def probe_batch(count=64, size=256, repeats=5):
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(count)
    first = rng.integers(0, 256, (count, size, size, 4), dtype=np.uint8)
    sampler = dict(srgb=True, linear=True, address_u=F.ADDRESS_REPEAT, address_v=F.ADDRESS_REPEAT)
    paths = contexts(lambda t: t + [dict(sampler, rgba=first[k]) for k in range(count)])
    own = len(paths["a"]["eng"]._textures) - count
    base = torch.from_numpy(first).to(dev)
    torch.cuda.synchronize()
    rows = {"a": [], "b": []}
    for r in range(repeats + 2):
        tensor = base + (r + 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = tensor.cpu().numpy()
        for k in range(count):
            paths["a"]["eng"].update_texture(own + k, dict(sampler, rgba=host[k]))
        t1 = time.perf_counter()
        paths["a"]["eng"].wait()
        t2 = time.perf_counter()
        paths["b"]["eng"].update_textures([dict(index=own + k, tensor=tensor[k]) for k in range(count)])
        t3 = time.perf_counter()
        paths["b"]["eng"].wait()
        t4 = time.perf_counter()
        if r >= 2:
            rows["a"].append((1e3 * (t1 - t0), 1e3 * (t2 - t0)))
            rows["b"].append((1e3 * (t3 - t2), 1e3 * (t4 - t2)))
    items, launches, texels = paths["b"]["eng"].last_texture_update()
    same = all(bool(np.array_equal(paths["a"]["eng"].read_texture(own + k), paths["b"]["eng"].read_texture(own + k))) for k in (0, count // 2, count - 1))
    med = lambda name, k: round(float(np.median([row[k] for row in rows[name]])), 4)
    out = {"batch": f"{count} textures of {size} x {size}, uint8 HWC", "host_path_calls": count, "host_path_launches": count,
           "host_path_call_ms": med("a", 0), "host_path_to_device_idle_ms": med("a", 1),
           "device_path_calls": 1, "device_path_items": items, "device_path_launches": launches, "device_path_texels": texels,
           "device_path_call_ms": med("b", 0), "device_path_to_device_idle_ms": med("b", 1), "both_paths_left_the_same_texels": same}
    for p in paths.values():
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
    for size in [int(a) for a in args] or [1024, 4096]:
        for kind in ("uint8_hwc", "float32_chw"):
            row = probe(size, kind, repeats)
            print(json.dumps(row), flush=True)
            rows.append(row)
    batch = probe_batch(repeats=repeats)
    print(json.dumps(batch), flush=True)
    if path:
        with open(path, "w") as fh:
            json.dump({"probe": "tools/texture_source_probe.py", "rows": rows, "batch": batch}, fh, indent=1)
