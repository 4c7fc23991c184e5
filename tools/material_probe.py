#!/usr/bin/env python3
"""Material and texture edits: the host path against the device path, in the same run.
  materials  synthetic_large with 2 000 / 20 000 instances (8 / 1 500 emitters), ONE material per instance.  Per edit - 1 % and 100 % of
             the materials, half of the emitters' materials among them with the emitter set unchanged (case A), and one emitter
             switched off / on (case B) - two contexts over twin builders take
               host    hk_upload_materials + hk_scene_builder_finish + hk_upload_scene_instances (the whole region laid out again), and
               device  hk_update_materials,
             alternately; reported: host time of the call(s), and the time from the call to the end of the next frame (hk_frame_wait).
             SceneBuilder.set_material expresses the edit on both builders and is timed apart.
  texture    hk_update_texture of one 1024 x 1024 image against hk_upload_textures of the array of four.
One process per step, each under its own time limit.  Not part of bench.py.
Usage: python tools/material_probe.py [--out FILE] [step ...]      steps: materials_2000 materials_20000 texture"""
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
from bevy_hikari_amd.scenes import synthetic_camera, synthetic_large, synthetic_scene

STEPS = {"materials_2000": 420, "materials_20000": 900, "texture": 300}   # seconds each may take
EMITTERS = {2000: 8, 20000: 1500}
REPS = 7


def one_material_per_instance(n_instances):
    """synthetic_large's scene with as many plain materials as instances, instance i (1..n) given material i (0 = the ground's)."""
    scene, sun = synthetic_large(0x5EED0004, 20, 16, 32, n_instances, n_instances + 1, EMITTERS[n_instances], 40.0)
    b = scene.builder
    for i in range(1, n_instances + 1):
        b.set_instance_material(i, i)
    scene = b.finish()
    scene.builder = b
    return scene, sun


def copy_of(m):
    out = F.HkMaterial()
    C.memmove(C.byref(out), C.byref(m), C.sizeof(F.HkMaterial))
    return out


def median_ms(v):
    return round(float(np.median(v)) * 1e3, 3)


def materials_step(n_instances):
    scenes = [one_material_per_instance(n_instances) for _ in range(2)]
    sun = scenes[0][1]
    host_scene, dev_scene = scenes[0][0], scenes[1][0]
    cam, s = synthetic_camera(1280, 720, extent=30.0), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    lights = hk.lights_uniform(directional=sun)
    n_mat = len(host_scene.materials)
    plain, emitter_ids = np.arange(0, n_instances + 1), np.arange(n_instances + 1, n_mat)
    assert len(emitter_ids) == EMITTERS[n_instances] == len(host_scene.emissives)
    materials = [copy_of(m) for m in host_scene.materials]
    warm = hk.HikariPlugin(device=0)   # (a process's first context renders faster than its later ones: neither timed context is the first)
    warm.set_scene(host_scene)
    warm.render(cam, s, lights=lights, frame_number=1)
    warm.engine.wait()
    host, dev = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    for p, sc in ((host, host_scene), (dev, dev_scene)):
        p.set_scene(sc)
        for n in (1, 2, 3):
            p.render(cam, s, lights=lights, frame_number=n)
        p.engine.wait()
    frame = [3]
    rng = np.random.default_rng(5)
    out = {"instances": len(host_scene.instances), "materials": n_mat, "emitters": len(emitter_ids), "triangles": len(host_scene.primitives)}

    def static_frame(p):
        t = []
        for _ in range(REPS):
            frame[0] += 1
            t0 = time.perf_counter()
            p.render(cam, s, lights=lights, frame_number=frame[0])
            p.engine.wait()
            t.append(time.perf_counter() - t0)
        return median_ms(t)

    out["frame_ms_without_edit"] = {"host": static_frame(host), "device": static_frame(dev)}

    def edit(ids, rep, emitters_on=None):
        """new values of materials `ids` on both builders; returns the seconds SceneBuilder.set_material took (per builder)"""
        t = 0.0
        for i in ids:
            m = materials[int(i)]
            if i in emitter_set:
                on = emitters_on is None or emitters_on
                m.emissive[:] = [0.3 + 0.05 * rep, 0.9 - 0.04 * rep, 0.6, 0.5 + 0.03 * rep] if on else [0.0, 0.0, 0.0, 1.0]
            else:
                m.base_color[:] = [0.2 + 0.07 * rep, 0.8 - 0.05 * rep, float(rng.uniform(0.1, 0.9)), 1.0]
                m.perceptual_roughness = 0.3 + 0.05 * rep
            t0 = time.perf_counter()
            host_scene.builder.set_material(int(i), m)
            t += time.perf_counter() - t0
            dev_scene.builder.set_material(int(i), m)
        return t

    emitter_set = set(int(i) for i in emitter_ids)

    def measure(name, pick, emitters_on=None):
        call = {"host": [], "device": []}
        to_frame_end = {"host": [], "device": []}
        set_ms, changed = [], 0
        for rep in range(REPS + 1):   # (the first repetition warms both paths up: staging, side arrays)
            ids = pick(rep)
            set_ms.append(edit(ids, rep, None if emitters_on is None else emitters_on(rep)))
            frame[0] += 1
            arr = (F.HkMaterial * n_mat)(*materials)
            for which, p in (("host", host), ("device", dev)) if rep % 2 else (("device", dev), ("host", host)):
                p.engine.wait()
                t0 = time.perf_counter()
                if which == "host":
                    b = host_scene.builder
                    p.engine.api.call("upload_materials", p.engine.ctx, arr, n_mat)
                    b.api.call("scene_builder_finish", b.h)
                    p.engine.api.call("upload_scene_instances", p.engine.ctx, b.h)
                else:
                    changed = p.engine.update_materials(dev_scene.builder, F.TREE_SAH)
                t1 = time.perf_counter()
                p.render(cam, s, lights=lights, frame_number=frame[0])
                p.engine.wait()
                t2 = time.perf_counter()
                if rep:
                    call[which].append(t1 - t0)
                    to_frame_end[which].append(t2 - t0)
        out[name] = {"records_changed": int(changed), "set_material_ms": median_ms(set_ms[1:]),
                     "host": {"call_ms": median_ms(call["host"]), "call_to_frame_end_ms": median_ms(to_frame_end["host"])},
                     "device": {"call_ms": median_ms(call["device"]), "call_to_frame_end_ms": median_ms(to_frame_end["device"])}}

    half_emitters = emitter_ids[::2]
    one_percent = np.concatenate([rng.choice(plain, size=max(1, n_mat // 100), replace=False), half_emitters[:max(1, len(half_emitters) // 100)]])
    measure("case_a_1_percent", lambda rep: one_percent)
    measure("case_a_1_percent_base_colours_only", lambda rep: one_percent[: max(1, n_mat // 100)])
    measure("case_a_100_percent", lambda rep: np.concatenate([plain, half_emitters]))
    measure("case_b_one_emitter_toggled", lambda rep: emitter_ids[1:2], emitters_on=lambda rep: rep % 2 == 1)
    st = dev.engine.stats()
    out["device_stats"] = {"instance_builds": int(st.scene_instance_builds), "device_tree_builds": int(st.scene_device_tree_builds)}
    return out


def texture_step():
    scene, sun = synthetic_scene(textured=True)
    rng = np.random.default_rng(9)
    images = [dict(t, rgba=rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8)) for t in scene.textures]
    scene.textures = images
    cam, s = synthetic_camera(1280, 720), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    lights = hk.lights_uniform(directional=sun)
    warm = hk.HikariPlugin(device=0)
    warm.set_scene(scene)
    warm.render(cam, s, lights=lights, frame_number=1)
    warm.engine.wait()
    host, dev = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    for p in (host, dev):
        p.set_scene(scene)
        for n in (1, 2, 3):
            p.render(cam, s, lights=lights, frame_number=n)
        p.engine.wait()
    call = {"host": [], "device": []}
    to_frame_end = {"host": [], "device": []}
    for rep in range(REPS + 1):
        images[1] = dict(images[1], rgba=rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8))
        for which, p in (("host", host), ("device", dev)) if rep % 2 else (("device", dev), ("host", host)):
            p.engine.wait()
            t0 = time.perf_counter()
            if which == "host":
                p.engine.upload_textures(images)
            else:
                p.engine.update_texture(1, images[1])
            t1 = time.perf_counter()
            p.render(cam, s, lights=lights, frame_number=4 + rep)
            p.engine.wait()
            t2 = time.perf_counter()
            if rep:
                call[which].append(t1 - t0)
                to_frame_end[which].append(t2 - t0)
    return {"images": 4, "size": [1024, 1024],
            "host_upload_textures": {"call_ms": median_ms(call["host"]), "call_to_frame_end_ms": median_ms(to_frame_end["host"])},
            "device_update_texture": {"call_ms": median_ms(call["device"]), "call_to_frame_end_ms": median_ms(to_frame_end["device"])}}


def child(step):
    if step == "texture":
        return texture_step()
    return materials_step(int(step.split("_")[1]))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print("RESULT " + json.dumps(child(args[1])), flush=True)
        sys.exit(0)
    out_path = os.path.join(ROOT, "profiles", "material_probe.json")
    if args[:1] == ["--out"]:
        out_path, args = args[1], args[2:]
    results = {}
    for step in args or list(STEPS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            results[step] = {"error": f"no result within {STEPS[step]} s"}
            print(json.dumps({step: results[step]}), flush=True)
            break   # (a step that hung: nothing more is started on this device)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            results[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-800:]}
            print(json.dumps({step: results[step]}), flush=True)
            break   # (nothing more is started after a step that failed)
        results[step] = json.loads(line[-1][len("RESULT "):])
        print(json.dumps({step: results[step]}), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
