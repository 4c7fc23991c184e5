"""Host-side constants of the reference compared with what the C ABI produces: the 3x3 a-trous kernel and the 16-entry Halton table
of FrameUniform (view.rs:125-140), HikariSettings::default() (lib.rs:435-455), the workgroup size and noise tile count (lib.rs).
The reference's values were read from its Rust / WGSL text (no Rust toolchain: parsed, not executed) into the data fixture
tests/golden/reference_constants.json by tests/tools/reference_constants.py; where a reference checkout is at hand
(HIKARI_REFERENCE_DIR, else its usual place) the fixture is also re-derived from it."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import reference_constants

REF = json.load(open(reference_constants.FIXTURE))


def test_frame_uniform_kernel_and_halton_table():
    kernel, halton = REF["frame_uniform"]["kernel"], REF["frame_uniform"]["halton"]
    assert len(kernel) == 9 and len(halton) == 32
    f = hk.frame_uniform(hk.HikariSettings(), 7)
    assert [float(f.kernel[c][r]) for c in range(3) for r in range(3)] == [float(np.float32(v)) for v in kernel]      # Mat3 columns x_axis, y_axis, z_axis
    assert [float(f.halton[i][k]) for i in range(8) for k in range(4)] == [float(np.float32(v)) for v in halton]
    assert f.number == 7


def test_settings_default():
    want = REF["settings_default"]
    s = F.HkSettings()
    F.api().call("settings_default", C.byref(s))
    for name in ("direct_validate_interval", "emissive_validate_interval", "max_temporal_reuse_count", "max_spatial_reuse_count", "indirect_bounces"):
        assert getattr(s, name) == int(want[name]), name
    for name in ("max_reservoir_lifetime", "solar_angle", "max_indirect_luminance"):
        assert float(getattr(s, name)) == float(np.float32(float(want[name]))), name
    for name in ("temporal_reuse", "emissive_spatial_reuse", "indirect_spatial_reuse", "denoise"):
        assert bool(getattr(s, name)) == want[name], name
    assert [float(c) for c in s.clear_color] == [float(np.float32(v)) for v in want["clear_color"]] + [1.0]
    # Taa::default() = Jasmine, Upscale::default() = SmaaTu4x { ratio: 2.0 } (lib.rs:466-496)
    assert REF["taa_default_is_jasmine"] and (s.taa, s.upscale_kind, s.upscale_ratio) == (F.TAA_JASMINE, F.UPSCALE_SMAA_TU4X, 2.0)
    assert REF["upscale_default_is_smaa_tu4x_ratio_2"]


def test_workgroup_size_noise_count_and_shader_constants():
    assert REF["workgroup_size"] == 8
    assert REF["noise_texture_count"] == 16
    light = REF["light_wgsl"]
    assert (light["RAY_BIAS"], light["DISTANCE_MAX"], light["MAX_VARIANCE"]) == (0.02, 65535.0, 10.0)


@pytest.mark.skipif(not os.path.isdir(reference_constants.REFERENCE_DIR), reason="no reference checkout (HIKARI_REFERENCE_DIR)")
def test_fixture_matches_the_reference_text():
    assert reference_constants.extract(reference_constants.REFERENCE_DIR) == REF
