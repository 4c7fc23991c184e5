#!/usr/bin/env python3
"""Host-side constants of the reference, read from its Rust / WGSL text (no Rust toolchain: parsed, not executed), stored as the data
fixture tests/golden/reference_constants.json that tests/test_reference_constants.py compares with the C ABI.

  [HIKARI_REFERENCE_DIR=<bevy-hikari checkout>] python tests/tools/reference_constants.py [--write]"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_constants.json")
REFERENCE_DIR = os.environ.get("HIKARI_REFERENCE_DIR") or "/root/reference"   # (the reference checkout: not part of this repository)


def numbers(text):
    return [float(x) for x in re.findall(r"-?\d+\.\d+", text)]


def extract(ref):
    """The constants, from the checkout at `ref`: the 3x3 a-trous kernel and the Halton table of FrameUniform (view.rs),
    HikariSettings::default() and the Taa / Upscale defaults (lib.rs), WORKGROUP_SIZE / NOISE_TEXTURE_COUNT (lib.rs), three
    constants of light.wgsl."""
    src = os.path.join(ref, "src")
    view = open(os.path.join(src, "view.rs")).read()
    lib = open(os.path.join(src, "lib.rs")).read()
    light = open(os.path.join(src, "shaders", "light.wgsl")).read()
    body = re.search(r"impl Default for HikariSettings \{.*?Self \{(.*?)\n        \}", lib, re.S).group(1)
    fields = dict(re.findall(r"(\w+): ([\w.:()\s,]+?),\n", body))
    settings = {}
    for name in ("direct_validate_interval", "emissive_validate_interval", "max_temporal_reuse_count", "max_spatial_reuse_count", "indirect_bounces"):
        settings[name] = int(fields[name])
    for name in ("max_reservoir_lifetime", "solar_angle", "max_indirect_luminance"):
        settings[name] = float(fields[name])
    for name in ("temporal_reuse", "emissive_spatial_reuse", "indirect_spatial_reuse", "denoise"):
        settings[name] = fields[name] == "true"
    settings["clear_color"] = numbers(fields["clear_color"])
    consts = dict(re.findall(r"^let (\w+): \w+ = ([^;]+);", light, re.M))
    return {
        "frame_uniform": {"kernel": numbers(re.search(r"const KERNEL: Mat3 = Mat3 \{(.*?)\};", view, re.S).group(1)),
                          "halton": numbers(re.search(r"const HALTON: \[Vec4; 8\] = \[(.*?)\];", view, re.S).group(1))},
        "settings_default": settings,
        "taa_default_is_jasmine": bool(re.search(r"#\[default\]\s*Jasmine", lib)),
        "upscale_default_is_smaa_tu4x_ratio_2": bool(re.search(r"SMAA_TU_2_0: Self = Self::SmaaTu4x \{ ratio: 2\.0 \}", lib) or re.search(r"SmaaTu4x \{ ratio: 2\.0 \}", lib)),
        "workgroup_size": int(re.search(r"pub const WORKGROUP_SIZE: u32 = (\d+);", lib).group(1)),
        "noise_texture_count": int(re.search(r"pub const NOISE_TEXTURE_COUNT: usize = (\d+);", lib).group(1)),
        "light_wgsl": {k: float(consts[k]) for k in ("RAY_BIAS", "DISTANCE_MAX", "MAX_VARIANCE")},
    }


if __name__ == "__main__":
    if not os.path.isdir(REFERENCE_DIR):
        sys.exit("no reference checkout at %s (HIKARI_REFERENCE_DIR names one)" % REFERENCE_DIR)
    data = extract(REFERENCE_DIR)
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")
    print(json.dumps(data, indent=1))
