"""The boundary of the device-source deformation (hk_deform_meshes_device, HkMeshDeformDevice, HK_DEFORM_RECOMPUTE_NORMALS) as every layer
states it, and the host twin of the recomputed normals (hk_scene_builder_recompute_mesh_normals) against the rule restated in numpy
float32 (deform_device_cases.py) bit for bit - no device needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.scenes import standard_material
from conftest import ROOT
from deform_device_cases import CASES, face_vectors, mesh_of, recomputed_normals

HEADER = os.path.join(ROOT, "include", "hikari_hip.h")


def header_text():
    return " ".join(re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S).split())


# ---- the boundary
def test_header_declares_both_functions_and_the_struct():
    text = header_text()
    assert "int hk_deform_meshes_device(hk_ctx* ctx, const HkMeshDeformDevice* items, uint32_t n, void* producer_stream);" in text
    assert "int hk_scene_builder_recompute_mesh_normals(hk_scene_builder* b, uint32_t mesh_id);" in text
    assert "#define HK_DEFORM_RECOMPUTE_NORMALS 1u" in text
    body = re.search(r"typedef struct HkMeshDeformDevice \{(.*?)\} HkMeshDeformDevice;", text)
    assert body, "HkMeshDeformDevice is not declared"
    fields = [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()]
    assert fields == ["HkMeshIndex mesh", "uint32_t kind", "uint32_t count", "const void* data", "const void* normals", "uint32_t data_stride",
                      "uint32_t normals_stride", "uint32_t flags", "uint32_t _pad"]


def test_ctypes_struct_has_the_headers_size_and_offsets():
    assert C.sizeof(F.HkMeshDeformDevice) == 56
    offsets = {name: getattr(F.HkMeshDeformDevice, name).offset for name, _ in F.HkMeshDeformDevice._fields_}
    assert offsets == dict(mesh=0, kind=16, count=20, data=24, normals=32, data_stride=40, normals_stride=44, flags=48, _pad=52)
    assert F.DEFORM_RECOMPUTE_NORMALS == 1
    assert F._PRODUCT_ONLY["deform_meshes_device"] == [C.c_void_p, C.POINTER(F.HkMeshDeformDevice), F.u32, C.c_void_p]
    assert F._PRODUCT_ONLY["scene_builder_recompute_mesh_normals"] == [C.c_void_p, F.u32]
    assert "hk_deform_meshes_device" in F.DECLARED_SYMBOLS and "hk_scene_builder_recompute_mesh_normals" in F.DECLARED_SYMBOLS
    for name in ("hk_deform_meshes_device", "hk_scene_builder_recompute_mesh_normals"):
        assert hasattr(F.api().dll, name), name


def test_generated_rust_crate_is_current_and_carries_the_call():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    assert "pub fn hk_deform_meshes_device(ctx: *mut HkCtx, items: *const HkMeshDeformDevice, n: u32, producer_stream: *mut c_void) -> i32;" in rust
    assert "pub fn hk_scene_builder_recompute_mesh_normals(b: *mut HkSceneBuilder, mesh_id: u32) -> i32;" in rust
    assert "size_of::<HkMeshDeformDevice>() == 56" in rust and "pub const HK_DEFORM_RECOMPUTE_NORMALS: u32 = 1;" in rust
    body = re.search(r"pub struct HkMeshDeformDevice \{(.*?)\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [name for name, _ in F.HkMeshDeformDevice._fields_]


def test_abi_version_stays_8_and_the_entry_point_answers_without_a_device():
    api = F.api()
    assert api.abi_version() == 8
    items = (F.HkMeshDeformDevice * 1)()
    assert api.raw("deform_meshes_device")(None, items, 1, None) == F.HK_E_INVALID
    assert api.raw("deform_meshes_device")(None, None, 0, None) == F.HK_E_INVALID
    assert api.raw("scene_builder_recompute_mesh_normals")(None, 0) == F.HK_E_INVALID
    # (n == 0 with a context is HK_OK: test_deform_device_gpu.py, where a context can exist)


def test_python_layers_offer_the_device_path():
    from bevy_hikari_amd.plugin import deform_items_device  # noqa: F401

    assert callable(getattr(hk.SceneBuilder, "recompute_mesh_normals", None))
    import inspect

    assert "producer_stream" in inspect.signature(hk.Engine.deform_meshes).parameters
    for text in (open(os.path.join(ROOT, "include", "hikari.hpp")).read(),):
        assert "hk_deform_meshes_device(" in text


# ---- the builder twin
def build(names):
    """one builder with the named cases as meshes (one instance each), finished: (builder, {name: (case, id, index)})"""
    b = hk.SceneBuilder()
    mat = b.add_material(standard_material((0.5, 0.5, 0.5, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
    meshes = {}
    for k, name in enumerate(names):
        case = CASES[name]()
        mid = b.add_mesh(case["positions"], case["normals"], case["uvs"], case["indices"], case["topology"])
        t = np.eye(4, dtype=np.float32)
        t[0, 3] = 2.5 * k
        b.add_instance(mid, mat, t.T.reshape(-1))
        meshes[name] = [case, mid, None]
    b.finish()
    for m in meshes.values():
        m[2] = b.mesh_index(m[1])
    return b, meshes


@pytest.fixture(scope="module")
def twin():
    """every case moved (set_mesh_vertices with normals NULL), recomputed and finished again: (scene, meshes, {name: (expected, kept, faces)})"""
    b, meshes = build(list(CASES))
    before = b.scene()
    expected = {}
    for name, (case, mid, index) in meshes.items():
        _p, current, tris = mesh_of(before, index, len(case["positions"]))
        assert np.array_equal(current, case["normals"])
        b.set_mesh_vertices(mid, case["moved"])
        b.recompute_mesh_normals(mid)
        expected[name] = recomputed_normals(case["moved"], tris, current) + (face_vectors(case["moved"], tris), tris)
    scene = b.finish()
    return scene, meshes, expected


@pytest.mark.parametrize("name", list(CASES))
def test_twin_equals_the_float32_restatement_bit_for_bit(twin, name):
    scene, meshes, expected = twin
    case, _mid, index = meshes[name]
    want, kept, faces, tris = expected[name]
    positions, normals, _ = mesh_of(scene, index, len(case["positions"]))
    assert positions.tobytes() == case["moved"].tobytes()
    assert normals.tobytes() == want.tobytes(), np.abs(normals - want).max()
    assert np.isfinite(normals).all()
    assert not kept.all(), "the case must recompute something"


def test_the_cases_hold_what_they_are_named_for(twin):
    scene, meshes, expected = twin
    _want, kept, faces, tris = expected["bent_grid"]
    assert len(tris) == 512 and len(kept) == 289 and not kept.any()
    assert (np.abs(faces[:, [0, 2]]).max(axis=1) / np.abs(faces[:, 1])).max() > 0.3      # bent: far from all +Y
    want, kept, faces, tris = expected["hub_fan"]
    assert (tris == 0).sum() == 40 and not kept[0]
    want, kept, faces, tris = expected["zero_area"]
    assert (faces == 0).all(axis=1).sum() == 1 and list(np.flatnonzero(kept)) == [5]          # vertex 5: named by the zero-area triangle alone
    assert want[5].tobytes() == meshes["zero_area"][0]["normals"][5].tobytes()
    want, kept, faces, tris = expected["unnamed_vertex"]
    assert 2 not in tris and list(np.flatnonzero(kept)) == [2] and want[2].tobytes() == meshes["unnamed_vertex"][0]["normals"][2].tobytes()
    want, kept, faces, tris = expected["strip"]
    assert len(tris) == 9
    want, kept, faces, tris = expected["minus_zero"]
    assert len(tris) == 1 and np.signbit(faces[0]).any() and (faces[0][np.signbit(faces[0])] == 0).all(), faces     # a face component of -0 ...
    assert not np.signbit(want).any() and not kept.any()                                                      # ... stored as +0


def test_twin_agrees_with_float64_after_normalisation(twin):
    """The numpy float32 restatement against the same sums in float64, both normalised: the largest deviation of any component over all
    six cases is what the twin is allowed - it is bit-equal to the restatement, so this only guards the restatement.  Measured on these
    inputs: 1.509e-07 (about one float32 ulp of a unit component)."""
    scene, meshes, expected = twin
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    allowed, worst = 0.0, 0.0
    for name, (case, _mid, index) in meshes.items():
        want, kept, _faces, tris = expected[name]
        exact, kept64 = recomputed_normals(case["moved"].astype(np.float64), tris, case["normals"].astype(np.float64), np.float64)
        assert np.array_equal(kept, kept64)
        _p, normals, _ = mesh_of(scene, index, len(case["positions"]))
        allowed = max(allowed, float(np.abs(unit(want.astype(np.float64)) - unit(exact))[~kept].max()))
        worst = max(worst, float(np.abs(unit(normals.astype(np.float64)) - unit(exact))[~kept].max()))
    print(f"float32 restatement against float64, normalised: {allowed:.3e}; the twin: {worst:.3e}")
    assert allowed < 1e-5, "the restatement itself is off"
    assert worst <= allowed


def test_recompute_leaves_instances_alone_and_the_next_finish_succeeds():
    b, meshes = build(["bent_grid", "hub_fan"])
    before = b.scene()
    b.recompute_mesh_normals(meshes["bent_grid"][1])          # positions as added: boxes and instance records must not move
    with pytest.raises(F.HikariError):
        b.mesh_index(meshes["bent_grid"][1])                     # the mesh level is un-finished, as after set_mesh_vertices
    after = b.finish()
    assert bytes(after.instances) == bytes(before.instances) and bytes(after.instance_nodes) == bytes(before.instance_nodes)
    assert bytes(after.asset_nodes) == bytes(before.asset_nodes) and bytes(after.primitives) == bytes(before.primitives)
    case, _mid, index = meshes["hub_fan"]
    assert mesh_of(after, index, 41)[1].tobytes() == case["normals"].tobytes()                # the other mesh is untouched
    _p, normals, tris = mesh_of(after, meshes["bent_grid"][2], 289)
    want, _ = recomputed_normals(meshes["bent_grid"][0]["positions"], tris, meshes["bent_grid"][0]["normals"])
    assert normals.tobytes() == want.tobytes()


def test_unknown_mesh_id_is_refused_with_the_builder_untouched():
    b, meshes = build(["hub_fan"])
    before = b.scene()
    assert b.api.raw("scene_builder_recompute_mesh_normals")(b.h, 1) == F.HK_E_INVALID
    assert "unknown mesh id" in b.api.last_error()
    assert bytes(b.mesh_index(meshes["hub_fan"][1])) == bytes(meshes["hub_fan"][2])             # still finished
    after = b.scene()
    for field in hk.SceneData.FIELDS:
        assert bytes(getattr(after, field)) == bytes(getattr(before, field)), field


# ---- the twin under the sanitizers: a stand-alone host program, nothing loaded into Python
def test_twin_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "bevy-hikari_amd", "csrc")
    prog = str(tmp_path / "recompute_normals")
    # (the runtimes linked into the program itself: it needs nothing from its environment)
    cmd = [gxx, "-O0", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"),
           "-o", prog, os.path.join(ROOT, "tests", "native", "recompute_normals_main.cpp"), os.path.join(csrc, "scene_builder.cpp"), os.path.join(csrc, "host_logic.cpp")]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan|static-lib", done.stderr):
        pytest.skip("this g++ has no sanitizer runtimes")
    assert done.returncode == 0, done.stderr[-2000:]
    run = subprocess.run([prog], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr[-4000:]
