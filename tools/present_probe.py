#!/usr/bin/env python3
"""Times k_present alone (HIP events around each launch, on the context's stream) against a streaming copy of the same number of
bytes measured in the same process (hk_measure_hbm), and writes profiles/present_probe.json.

    python tools/present_probe.py [--out profiles/present_probe.json]

Cases: a 1920 x 1080 target from a 1920 x 1080 source (both planes read at the texel), and a 3840 x 2160 target from a 1920 x 1080
source (bilinear), each into bgra8-sRGB and rgba16f under HK_PRESENT_CLEAR.  Median of 200 launches after 50 warm-up launches;
beside it the mean of 200 launches back to back inside one event pair, which is how the copy itself is timed.
The kernel reads 8 B per source texel it touches and writes 4 or 8 B per target pixel; a ratio far above 1 means the albedo is
being read unconditionally or the stores are not coalesced."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, LAUNCHES = 50, 200


def main():
    import torch

    import bevy_hikari_amd as hk
    from bevy_hikari_amd import _ffi as F

    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "present_probe.json")
    plugin = hk.HikariPlugin(device=0)
    plugin.set_scene(hk.load_cornell())
    e = plugin.engine
    stream = torch.cuda.Stream()       # (not torch's default stream: its handle is 0, which hk_set_stream reads as "the context's own")
    e.set_stream(stream.cuda_stream)   # the events below are torch's: they have to be recorded on the stream the kernel runs on
    assert e.stream() == stream.cuda_stream
    results = []
    for name, window, ratio in (("1080p from 1080p", (1920, 1080), 1.0), ("2160p from 1080p", (3840, 2160), 2.0)):
        settings = hk.HikariSettings(upscale=hk.Upscale.SmaaTu4x(ratio))
        sc = settings.to_c()
        e.resize(*window, ratio)
        camera = hk.cornell_camera(*window)
        e.frame_begin(hk.frame_uniform(settings, 2), camera.view_uniform(), camera.previous_view_uniform(None), hk.lights_uniform())
        sw, sh, _ = e.buffer_info(F.BUF_TONE_MAPPED)
        W, H = window
        for fmt, code, dtype, pixel in (("bgra8-srgb", F.FORMAT_BGRA8_UNORM_SRGB, torch.uint8, 4), ("rgba16f", F.FORMAT_RGBA16F, torch.float16, 8)):
            target = torch.zeros((H, W, 4), dtype=dtype, device="cuda:0")
            torch.cuda.synchronize()
            times = []
            for k in range(WARMUP + LAUNCHES):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                e.present_into(sc, 0, target.data_ptr(), W, H, W * pixel, code, F.PRESENT_CLEAR, settings.clear_color)
                t1.record(stream)
                if k >= WARMUP:
                    times.append((t0, t1))
            torch.cuda.synchronize()
            ms = statistics.median(a.elapsed_time(b) for a, b in times)
            # the same launches back to back inside ONE event pair, as hk_measure_hbm times its copy: without the dispatch latency
            # (and hk_present's host work) that every pair above encloses - the like-for-like figure
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(LAUNCHES):
                e.present_into(sc, 0, target.data_ptr(), W, H, W * pixel, code, F.PRESENT_CLEAR, settings.clear_color)
            t1.record(stream)
            torch.cuda.synchronize()
            ms_b2b = t0.elapsed_time(t1) / LAUNCHES
            moved = sw * sh * 8 + W * H * pixel
            copy_gbs, _ = e.measure_hbm(bytes_per_array=moved // 2, reps=LAUNCHES)   # (a copy moves 2 x bytes_per_array: the same number of bytes)
            copy_ms = moved / (copy_gbs * 1e9) * 1e3
            results.append({"case": name, "format": fmt, "source": [sw, sh], "target": [W, H], "bytes_moved": moved, "k_present_ms_median": ms,
                            "k_present_gbs": moved / (ms * 1e-3) / 1e9, "copy_gbs_same_bytes": copy_gbs, "copy_ms_same_bytes": copy_ms,
                            "ratio_to_copy": ms / copy_ms, "k_present_ms_back_to_back": ms_b2b, "ratio_to_copy_back_to_back": ms_b2b / copy_ms})
            print(json.dumps(results[-1]), flush=True)
    e.set_stream(0)
    doc = {"tool": "tools/present_probe.py", "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "launches": LAUNCHES,
           "flags": "HK_PRESENT_CLEAR", "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
