"""Motion vectors for deforming meshes (hk_set_mesh_motion_vectors), the half that needs no GPU: the entry point as every layer declares it,
and its answers without a device."""
import ctypes as C
import inspect
import os
import re

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.distributed import MultiEngine
from conftest import ROOT


def text(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_symbol_is_declared_in_every_layer():
    header = text("include", "hikari_hip.h")
    assert re.search(r"\bint hk_set_mesh_motion_vectors\(hk_ctx\* ctx, const HkMeshIndex\* mesh, uint32_t enable\);", header)
    assert re.search(r"\bint hk_multi_set_mesh_motion_vectors\(hk_multi\* m, const HkMeshIndex\* mesh, uint32_t enable\);", header)
    assert re.search(r"\bint hk_debug_last_motion\(hk_ctx\* ctx, uint32_t out\[3\]\);", text("include", "hikari_hip_debug.h"))
    rust = text("rust", "hikari-hip-sys", "src", "lib.rs")
    assert "pub fn hk_set_mesh_motion_vectors(ctx: *mut HkCtx, mesh: *const HkMeshIndex, enable: u32) -> i32;" in rust
    assert "pub fn hk_multi_set_mesh_motion_vectors(m: *mut HkMulti, mesh: *const HkMeshIndex, enable: u32) -> i32;" in rust
    api = hk.api()
    for name in ("set_mesh_motion_vectors", "multi_set_mesh_motion_vectors", "debug_last_motion"):
        assert api.raw(name) is not None
    cpp = text("include", "hikari.hpp")
    assert cpp.count("set_mesh_motion_vectors(const HkMeshIndex& mesh, bool enabled = true)") == 2   # HikariPlugin and HikariMultiGpuPlugin


def test_the_abi_version_stays_8():
    assert re.search(r"#define\s+HK_ABI_VERSION\s+8u?\b", text("include", "hikari_hip.h"))
    assert hk.api().abi_version() == 8


def test_the_entry_point_answers_without_a_device():
    api = hk.api()
    mesh = F.HkMeshIndex()
    for ctx, m in ((None, C.byref(mesh)), (None, None)):
        assert api.raw("set_mesh_motion_vectors")(ctx, m, 1) == F.HK_E_INVALID
        assert "NULL" in api.last_error()
    assert api.raw("multi_set_mesh_motion_vectors")(None, C.byref(mesh), 1) == F.HK_E_INVALID
    out = (F.u32 * 3)()
    assert api.raw("debug_last_motion")(None, out) == F.HK_E_INVALID


def test_the_python_layers_expose_the_call():
    for cls in (hk.Engine, hk.HikariPlugin, MultiEngine):
        sig = inspect.signature(cls.set_mesh_motion_vectors)
        assert list(sig.parameters) == ["self", "mesh", "enabled"] and sig.parameters["enabled"].default is True
    assert list(inspect.signature(hk.Engine.last_motion).parameters) == ["self"]
    assert F.DEBUG_OPT_MOTION_COUNT == 15
