#!/usr/bin/env python3
"""A skinned cylinder bending over 32 frames at 1280 x 720 in front of a static room (the small yard and a back wall; one bounce, ReSTIR +
denoise), rendered with and without hk_set_mesh_motion_vectors, at three sizes of the cylinder on screen.  Writes
profiles/motion_vector_probe.json:
 (a) per size: the cylinder's share of the screen, the time of the motion pass (k_motion_velocity), of the primary rays (k_prepass) and
     of the frame - HIP events through the context's statistics (hk_set_timing_mask: the prepass's slot and HK_TIMING_MOTION_VECTORS),
     medians over frames 9 .. 32, both arms under the same mask;
 (b) per frame: the share of the cylinder's pixels whose direct-light and indirect temporal reservoirs kept history - the f16 `count` of
     the record the temporal pass wrote (the reservoir buffer of the frame's parity) above 1.
Every arm runs in a child process of its own, one after the other (`--arm SCALE 0|1`): a process's first context and its later ones
do not get the same hardware queues, and the arms must not differ by their place in a queue.
`--rocprof` adds a child process of its own, `rocprofv3 --kernel-trace --stats -d DIR -- python tools/motion_vector_probe.py --trace`
(the feature's arm at the middle size, nothing read back), and reads the two kernels' durations from what it leaves.
Usage: python tools/motion_vector_probe.py [--out FILE] [--frames N] [--rocprof] [--trace] [--arm SCALE 0|1]"""
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = (1280, 720)
SCALES = [1.0, 2.2, 4.0]     # of the cylinder (0.3 across, 1.2 tall at 1.0)
WARM = 8                     # frames left out of the medians


def build_scene(scale):
    from bevy_hikari_amd import scenes as S

    scene, sun = S.synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    wall = b.add_mesh(*S._box())
    p, n, uv, idx, ji, jw = S.bending_cylinder()
    cyl = b.add_mesh(p, n, uv, idx)
    grey = b.add_material(S.standard_material((0.75, 0.75, 0.7, 1.0), (0, 0, 0), 0.8, 0.0, 0.5))
    red = b.add_material(S.standard_material((0.7, 0.2, 0.2, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
    b.add_instance(wall, grey, S._trs((0.0, 2.5, -4.5), (0, 0, 0), (14.0, 6.0, 0.3)))
    b.add_instance(cyl, red, S._trs((1.5, 0.0, 2.0), (0.0, 0.4, 0.0), (scale, scale, scale)))
    scene = b.finish()
    scene.builder = b
    return scene, sun, b.mesh_index(cyl), len(scene.instances) - 1, (p, n, ji, jw)


def history_share(engine, F, frame_number, instance):
    """share of `instance`'s pixels whose temporal reservoirs of this frame have count > 1: (direct light, indirect)"""
    im = engine.read(F.BUF_INSTANCE_MATERIAL)
    mask = (im[..., 0] > 0) & (np.floor(im[..., 0]) == instance)
    out = []
    for first in (0, 6):   # make_light_targets: the temporal pass of frame n writes buffer (1 - n % 2) + {0 sun, 2 emissive, 6 indirect}
        rec = engine.read(F.BUF_RESERVOIR0 + (1 - frame_number % 2) + first)
        count = (rec[..., 14] & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
        out.append(float((count[mask] > 1.0).mean()) if mask.any() else None)
    return int(mask.sum()), out


def run_arm(scale, enable, frames, read_back=True):
    import bevy_hikari_amd as hk
    from bevy_hikari_amd import _ffi as F
    from bevy_hikari_amd import scenes as S

    scene, sun, index, instance, (p, n, ji, jw) = build_scene(scale)
    plugin = hk.HikariPlugin(device=0)
    e = plugin.engine
    plugin.set_scene(scene)
    e.set_mesh_skin(index, p, n, ji, jw)
    if enable:
        plugin.set_mesh_motion_vectors(index)
    e.set_timing_mask((1 << F.PASS_PREPASS) | (1 << F.TIMING_MOTION_VECTORS))
    cam = S.synthetic_camera(*SIZE)
    lights = hk.lights_uniform(directional=sun)
    s = hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    per_frame, frame_ms, before = [], [], None
    for k in range(1, frames + 1):
        plugin.deform_meshes([("skin", index, S.bend_joints(0.25 * k))])
        plugin.render(cam, s, lights=lights, frame_number=k)
        e.wait()
        st = e.stats()
        now = (st.pass_ms_total[F.PASS_PREPASS], st.pass_launches[F.PASS_PREPASS], st.pass_ms_total[F.TIMING_MOTION_VECTORS], st.pass_launches[F.TIMING_MOTION_VECTORS])
        if k == WARM:
            before = now
        if k > WARM:
            frame_ms.append(float(st.last_frame_ms))
        if read_back:
            pixels, share = history_share(e, F, k, instance)
            per_frame.append({"frame": k, "mesh_pixels": pixels, "direct_kept": share[0], "indirect_kept": share[1], "motion": list(e.last_motion()[:2])})
    after = now
    d = [a - b for a, b in zip(after, before)]
    out = {"scale": scale, "motion_vectors": bool(enable), "frames_timed": frames - WARM,
           "prepass_ms": d[0] / max(d[1], 1), "motion_pass_ms": (d[2] / d[3]) if d[3] else None, "motion_pass_launches": int(d[3]),
           "frame_ms_median": float(np.median(frame_ms)), "frame_ms_range": [min(frame_ms), max(frame_ms)]}
    if read_back:
        out["coverage"] = per_frame[-1]["mesh_pixels"] / float(SIZE[0] * SIZE[1])
        tail = [f for f in per_frame if f["frame"] > WARM]
        out["direct_kept_mean"] = float(np.mean([f["direct_kept"] for f in tail]))
        out["indirect_kept_mean"] = float(np.mean([f["indirect_kept"] for f in tail]))
        out["per_frame"] = per_frame
    return out


def kernel_times(directory):
    """median duration (us) and count of k_motion_velocity and k_prepass dispatches in what rocprofv3 left under `directory`"""
    import sqlite3

    found = {}
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        db = sqlite3.connect(path)
        try:
            cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
            if not cols:
                continue
            start, end = ("start" if "start" in cols else "start_timestamp"), ("end" if "end" in cols else "end_timestamp")
            for name in ("k_motion_velocity", "k_prepass"):
                ns = [t1 - t0 for t0, t1 in db.execute(f"select {start}, {end} from kernels where name like '%{name}%' order by {start}")]
                if ns:
                    found[name] = {"dispatches": len(ns), "median_us": float(np.median(ns[WARM:] or ns)) / 1e3}
        finally:
            db.close()
    if not found:
        import csv

        for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
            rows = list(csv.DictReader(open(path)))
            for name in ("k_motion_velocity", "k_prepass"):
                ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r.get("Kernel_Name", "")]
                if ns:
                    found[name] = {"dispatches": len(ns), "median_us": float(np.median(ns[WARM:] or ns)) / 1e3}
    return found


if __name__ == "__main__":
    args = sys.argv[1:]
    path, frames, rocprof, trace, arm = os.path.join(ROOT, "profiles", "motion_vector_probe.json"), 32, False, False, None
    while args:
        if args[0] == "--out":
            path, args = args[1], args[2:]
        elif args[0] == "--frames":
            frames, args = int(args[1]), args[2:]
        elif args[0] == "--rocprof":
            rocprof, args = True, args[1:]
        elif args[0] == "--trace":
            trace, args = True, args[1:]
        elif args[0] == "--arm":
            arm, args = (float(args[1]), args[2] == "1"), args[3:]
        else:
            raise SystemExit(__doc__)
    if trace:   # (the child of --rocprof: the kernels alone)
        run_arm(SCALES[1], True, frames, read_back=False)
        sys.exit(0)
    if arm:     # (one arm, as the child of the run below: its record is the last line)
        print(json.dumps(run_arm(arm[0], arm[1], frames)), flush=True)
        sys.exit(0)
    result = {"size": list(SIZE), "frames": frames, "settings": "1 bounce, ReSTIR + denoise, ratio 1", "arms": []}
    for scale in SCALES:
        for enable in (False, True):
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", str(scale), "1" if enable else "0", "--frames", str(frames)], capture_output=True,
                                   text=True, timeout=180)
            if child.returncode != 0:
                raise SystemExit(f"arm {scale} {enable} failed: {child.stderr[-800:]}")
            record = json.loads(child.stdout.strip().splitlines()[-1])
            print(json.dumps({k: v for k, v in record.items() if k != "per_frame"}), flush=True)
            result["arms"].append(record)
    if rocprof:
        out_dir = os.path.join(os.path.dirname(os.path.abspath(path)), "motion_vector_trace")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--trace", "--frames", str(frames)]
        shown = "rocprofv3 --kernel-trace --stats -d DIR -- python tools/motion_vector_probe.py --trace --frames %d" % frames
        try:
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            result["rocprofv3"] = {"command": shown, "returncode": child.returncode,
                                   "scale": SCALES[1], "kernels": kernel_times(out_dir)}
            if child.returncode != 0:
                result["rocprofv3"]["stderr_tail"] = child.stderr[-600:]
        except Exception as err:   # (not measured: say why)
            result["rocprofv3"] = {"not_measured": repr(err)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)
