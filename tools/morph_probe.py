#!/usr/bin/env python3
"""One morphing grid mesh of 10^4, 10^5 and 10^6 vertices in the small yard (eight orderings, 960 x 540, one bounce), blended two ways on one
context, alternating in one run:
 (a) what a host does without the morph items: the blend on the host - hk_morph_vertices or the numpy blend (scenes.morph_reference),
     whichever is faster at that size - then a HK_DEFORM_VERTICES item carrying the blended positions and normals;
 (b) a HK_DEFORM_MORPH item carrying the weights alone.
Per size and configuration (targets in the set / targets active; the sets have normal deltas), medians over the repeats after two warm
rounds: the host time of the call (for (a) with the blend), the time from the start of the path to the end of the next frame, the device
time of batch (b) from HIP events on the context's stream with its range over the repeats.  `--trace` is the run for
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/morph_probe.py --trace ...` (a run of its own: batches (b) only, a fixed number
per configuration), `--parse DB` then reads k_deform_vertices' durations from the rocpd database, configuration by configuration, and
sets them against the bytes the launch must read and write at the achievable HBM rate (6.3 TB/s): the kernel's share of that bound.
Usage: python tools/morph_probe.py [--out FILE] [--repeats N] [--trace] [--parse DB] [VERTICES ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [(4, 4), (8, 4), (8, 8), (52, 4), (52, 52)]   # (targets in the set, targets active)
TRACE_BATCHES = 9                                        # per configuration in a --trace run; the first two are warm-up
HBM_BYTES_PER_S = 6.3e12                                 # achievable, float4 copy


def vertex_launch_bytes(nv, active, normal_deltas=True):
    """what k_deform_vertices must move for a morph item: both base planes, one delta plane (two with normal deltas) per ACTIVE target, the
    position and the normal written as float4"""
    return nv * (24 + active * (24 if normal_deltas else 12) + 32)


def weights_for(targets, active, k):
    w = np.zeros(targets, np.float32)
    on = np.arange(active) * targets // active   # spread over the set
    w[on] = 0.3 + 0.05 * np.sin(0.7 * k + on)
    return w


def grid_scene(side):
    from bevy_hikari_amd import scenes as S

    scene, sun = S.synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    p, n, uv, idx = S.cloth_grid(side - 1, side - 1, size=3.0)
    mesh = b.add_mesh(p, n, uv, idx)
    b.add_instance(mesh, b.add_material(S.standard_material((0.3, 0.6, 0.8, 1.0), (0, 0, 0), 0.6, 0.0, 0.5)), S._trs((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    return b.finish(), sun, b, mesh, p, n


def probe(vertices, repeats=5, trace=False):
    import torch

    import bevy_hikari_amd as hk
    from bevy_hikari_amd import _ffi as F
    from bevy_hikari_amd import scenes as S
    from bevy_hikari_amd.plugin import Camera, deform_items, look_at_transform

    side = max(2, int(round(vertices ** 0.5)))
    scene, sun, builder, mesh_id, rest, normals = grid_scene(side)
    index = builder.mesh_index(mesh_id)
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

    call = eng.api.raw("deform_meshes")
    rng = np.random.default_rng(vertices)
    most = max(t for t, _ in CONFIGS)
    all_dp = np.float32(0.02) * rng.standard_normal((most, nv, 3), dtype=np.float32)
    all_dn = np.float32(0.05) * rng.standard_normal((most, nv, 3), dtype=np.float32)
    mode, orderings = F.u32(), F.u32()
    eng.api.call("traversal_mode", eng.ctx, mode, orderings)
    rows = []
    for targets, active in CONFIGS:
        dp, dn = all_dp[:targets], all_dn[:targets]
        eng.set_mesh_morph_targets(index, rest, normals, dp, dn)

        def path_a(w, blend):
            t0 = time.perf_counter()
            pos, nrm = blend(rest, normals, dp, dn, w)
            t1 = time.perf_counter()
            table, keep = deform_items([("vertices", index, pos, nrm)])
            if call(eng.ctx, table, 1) != F.HK_OK:
                raise RuntimeError(eng.api.last_error())
            return t0, t1 - t0, time.perf_counter()

        def path_b(w):
            t0 = time.perf_counter()
            table, keep = deform_items([("morph", index, w)])
            if call(eng.ctx, table, 1) != F.HK_OK:
                raise RuntimeError(eng.api.last_error())
            return t0, 0.0, time.perf_counter()

        if trace:   # batches (b) alone, TRACE_BATCHES of them: --parse finds them again by their order
            for r in range(TRACE_BATCHES):
                path_b(weights_for(targets, active, r))
                frame()
                eng.wait()
            continue
        # which host blend is faster here: three runs of each, the best
        blends = {"hk_morph_vertices": hk.morph_vertices, "numpy": S.morph_reference}
        best = {}
        for name, blend in blends.items():
            times = []
            for r in range(3):
                t0 = time.perf_counter()
                blend(rest, normals, dp, dn, weights_for(targets, active, r))
                times.append(time.perf_counter() - t0)
            best[name] = min(times)
        blend_name = min(best, key=best.get)
        samples = {"a": [], "b": []}
        for r in range(repeats + 2):   # (the first two rounds warm both paths: refit planes, staging blocks)
            for name in ("a", "b"):
                w = weights_for(targets, active, 2 * r + (name == "b"))
                frame()
                eng.wait()
                t0, blend_s, t1 = path_a(w, blends[blend_name]) if name == "a" else path_b(w)
                frame()
                eng.wait()
                t2 = time.perf_counter()
                if r >= 2:
                    samples[name].append((1e3 * (t1 - t0), 1e3 * (t2 - t0), 1e3 * blend_s))
        launches = eng.last_deform()[3]
        device_ms = []
        for r in range(repeats + 2):   # the device time of batch (b) alone, from events on the context's stream
            eng.wait()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            path_b(weights_for(targets, active, r))
            e1.record(stream)
            e1.synchronize()
            if r >= 2:
                device_ms.append(e0.elapsed_time(e1))
        med = lambda v: round(float(np.median(v)), 4)
        col = lambda name, k: med([row[k] for row in samples[name]])
        rows.append({"vertices": nv, "triangles": 2 * (side - 1) ** 2, "targets": targets, "active": active, "orderings": int(orderings.value),
                     "host_blend": blend_name, "host_blend_ms": col("a", 2), "host_path_call_ms": col("a", 0), "host_path_to_frame_end_ms": col("a", 1),
                     "morph_call_ms": col("b", 0), "morph_to_frame_end_ms": col("b", 1), "morph_launches": launches,
                     "morph_batch_device_ms": med(device_ms), "morph_batch_device_ms_range": [round(min(device_ms), 4), round(max(device_ms), 4)],
                     "vertex_launch_bytes": vertex_launch_bytes(nv, active), "vertex_launch_hbm_bound_us": round(1e6 * vertex_launch_bytes(nv, active) / HBM_BYTES_PER_S, 2)})
        print(json.dumps(rows[-1]), flush=True)
    eng.wait()
    eng.set_stream(0)
    eng.close()
    return rows


def parse(db_path, sizes):
    """k_deform_vertices of a --trace run, in dispatch order: TRACE_BATCHES per configuration, per size"""
    import sqlite3

    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    start, end = ("start" if "start" in cols else "start_timestamp"), ("end" if "end" in cols else "end_timestamp")
    ns = [e - s for s, e in db.execute(f"select {start}, {end} from kernels where name like '%k_deform_vertices%' order by {start}")]
    db.close()
    if len(ns) != len(sizes) * len(CONFIGS) * TRACE_BATCHES:
        raise SystemExit(f"{len(ns)} k_deform_vertices dispatches, expected {len(sizes) * len(CONFIGS) * TRACE_BATCHES}")
    rows, at = [], 0
    for vertices in sizes:
        side = max(2, int(round(vertices ** 0.5)))
        nv = side * side
        for targets, active in CONFIGS:
            us = [t / 1e3 for t in ns[at + 2:at + TRACE_BATCHES]]
            at += TRACE_BATCHES
            bound = 1e6 * vertex_launch_bytes(nv, active) / HBM_BYTES_PER_S
            rows.append({"vertices": nv, "targets": targets, "active": active, "vertex_launch_us": round(float(np.median(us)), 2),
                         "vertex_launch_us_range": [round(min(us), 2), round(max(us), 2)], "vertex_launch_bytes": vertex_launch_bytes(nv, active),
                         "hbm_bound_us": round(bound, 2), "share_of_hbm_bound": round(bound / float(np.median(us)), 3)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    path, repeats, trace, db = None, 5, False, None
    while args and args[0].startswith("--"):
        if args[0] == "--trace":
            trace, args = True, args[1:]
            continue
        if args[0] == "--out":
            path = args[1]
        elif args[0] == "--repeats":
            repeats = int(args[1])
        elif args[0] == "--parse":
            db = args[1]
        else:
            raise SystemExit(__doc__)
        args = args[2:]
    sizes = [int(a) for a in args] or [10_000, 100_000, 1_000_000]
    if db:
        out = {"probe": "tools/morph_probe.py --parse", "vertex_launch": parse(db, sizes)}
    else:
        rows = []
        for n in sizes:
            rows += probe(n, repeats, trace)
        out = {"probe": "tools/morph_probe.py", "rows": rows}
    if path and not trace:
        old = {}
        if os.path.exists(path):
            with open(path) as fh:
                old = json.load(fh)
        old.update(out)
        old["probe"] = "tools/morph_probe.py"
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1)
