#!/usr/bin/env python3
"""Instance-set changes of a scene that holds one skinned mesh, at 2 000 and 20 000 instances: one instance spawned, 1 % despawned.

  change    hk_change_scene_instances (Engine.change_instances): the host lays the level out, the device derives what the mirrors hold stale
  baseline  what a host has to do WITHOUT that call.  After the mesh was skinned on the device: hk_scene_builder_finish + hk_upload_scene of
            the whole builder, then the skin set again and the mesh skinned again (hk_upload_scene drops it).  Before any deformation:
            hk_update_scene_instances.

Per edit and arm: the host time of the call(s), and the time from the call to the end of the next frame (call + one 1280 x 720 frame, waited
for).  Medians of REPEATS edits on one context per arm; the baselines never go through the new call.
    python tools/instance_change_probe.py [--out FILE] [n_instances ...]      writes profiles/instance_change_probe.json, or FILE"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.scenes import synthetic_camera, synthetic_large

REPEATS = 5


def build(n_instances):
    """(builder, mesh id of the skinned cylinder, its data, sun): few small unique meshes - the instance count is what is varied"""
    scene, sun = synthetic_large(0x5EED0004, 20, 16, 32, n_instances, 50, 8, 40.0)
    b = scene.builder
    p, n, uv, i, ji, jw = S.bending_cylinder()
    cyl = b.add_mesh(p, n, uv, i)
    b.add_instance(cyl, 1, S._trs((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)))
    return b, cyl, dict(positions=p, normals=n, joints=ji, weights=jw), sun


def skin(engine, b, cyl, d, frame):
    idx = b.mesh_index(cyl)
    engine.set_mesh_skin(idx, d["positions"], d["normals"], d["joints"], d["weights"])
    engine.deform_meshes([("skin", idx, S.bend_joints(frame))])


def arm(n_instances, state, which, edit):
    b, cyl, d, sun = build(n_instances)
    cam, s, lights = synthetic_camera(1280, 720, extent=30.0), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0), hk.lights_uniform(directional=sun)
    plugin = hk.HikariPlugin(device=0)
    e = plugin.engine
    scene = b.finish()
    plugin.set_scene(scene)
    b.take_origins()
    if state == "skinned":
        skin(e, b, cyl, d, 1)
    frame = 1
    plugin.render(cam, s, lights=lights, frame_number=frame)
    e.wait()
    rng = np.random.default_rng(3)
    pose = np.ctypeslib.as_array(scene.instances[1].model).copy()
    host, to_frame = [], []
    for r in range(REPEATS + 1):   # (the first edit is the cold one: allocations, pinned staging; left out of the medians)
        count = len(b.origins)
        if edit == "spawn_one":
            m = pose.copy()
            m[12] += 0.5 * (r + 1)
            b.add_instance(1, 1, m)
        else:
            for k in sorted(rng.choice(np.arange(1, count - 9), size=max(1, count // 100), replace=False).tolist(), reverse=True):
                b.remove_instance(int(k))
        e.wait()
        t0 = time.perf_counter()
        if which == "change":
            e.change_instances(b, F.TREE_SAH)
        elif state == "skinned":
            e.upload_scene(b.finish())
            skin(e, b, cyl, d, frame)
            b.take_origins()
        else:
            e.update_instances_on_device(b, F.TREE_SAH)
            b.take_origins()
        t1 = time.perf_counter()
        frame += 1
        plugin.render(cam, s, lights=lights, frame_number=frame)
        e.wait()
        t2 = time.perf_counter()
        if r:
            host.append((t1 - t0) * 1e3)
            to_frame.append((t2 - t0) * 1e3)
    out = dict(host_ms=round(float(np.median(host)), 3), call_to_frame_end_ms=round(float(np.median(to_frame)), 3), instances_after=len(b.origins))
    if which == "change":
        out["last_instance_change"] = list(e.last_instance_change())
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "instance_change_probe.json")
    if "--out" in args:
        at = args.index("--out")
        out_path = os.path.abspath(args[at + 1])
        del args[at:at + 2]
    sizes = [int(a) for a in args] or [2000, 20000]
    result = dict(frame="1280x720, indirect_bounces=1", repeats=REPEATS, scenes={})
    for n in sizes:
        rec = {}
        for state in ("skinned", "never_deformed"):
            for edit in ("spawn_one", "despawn_1pct"):
                rec[f"{state}/{edit}"] = {which: arm(n, state, which, edit) for which in ("change", "baseline")}
                print(n, state, edit, json.dumps(rec[f"{state}/{edit}"]), flush=True)
        result["scenes"][str(n)] = rec
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
