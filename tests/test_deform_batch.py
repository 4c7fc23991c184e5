"""The boundary of the batched deformation (hk_deform_meshes, hk_multi_deform_meshes, HkMeshDeform) as every layer states it: the header,
the ctypes mirror, the generated Rust crate, the library's export table - and what the entry points answer without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

from bevy_hikari_amd import _ffi as F
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hikari_hip.h")


def header_text():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def test_header_declares_both_functions_and_the_struct():
    text = " ".join(header_text().split())
    assert "int hk_deform_meshes(hk_ctx* ctx, const HkMeshDeform* items, uint32_t n);" in text
    assert "int hk_multi_deform_meshes(hk_multi* m, const HkMeshDeform* items, uint32_t n);" in text
    assert "#define HK_DEFORM_VERTICES 0u" in text and "#define HK_DEFORM_SKIN 1u" in text
    body = re.search(r"typedef struct HkMeshDeform \{(.*?)\} HkMeshDeform;", text)
    assert body, "HkMeshDeform is not declared"
    fields = [" ".join(f.split()) for f in body.group(1).split(";") if f.strip()]
    assert fields == ["HkMeshIndex mesh", "uint32_t kind", "uint32_t count", "const float* data", "const float* normals"]
    debug = open(os.path.join(ROOT, "include", "hikari_hip_debug.h")).read()
    assert "int hk_debug_last_deform(hk_ctx* ctx, uint32_t out[6]);" in debug


def test_ctypes_struct_has_the_headers_size_and_offsets():
    """HkMeshIndex (4 x u32) | kind | count | two pointers: 40 bytes under the C layout rules of the header's field order."""
    assert C.sizeof(F.HkMeshDeform) == 40
    offsets = [(name, getattr(F.HkMeshDeform, name).offset) for name, _ in F.HkMeshDeform._fields_]
    assert offsets == [("mesh", 0), ("kind", 16), ("count", 20), ("data", 24), ("normals", 32)]
    assert (F.DEFORM_VERTICES, F.DEFORM_SKIN) == (0, 1)
    assert F._PRODUCT_ONLY["deform_meshes"] == [C.c_void_p, C.POINTER(F.HkMeshDeform), F.u32]
    assert F._PRODUCT_ONLY["multi_deform_meshes"] == [C.c_void_p, C.POINTER(F.HkMeshDeform), F.u32]
    assert F._DEBUG["debug_last_deform"] == [C.c_void_p, C.POINTER(F.u32)]


def test_generated_rust_crate_is_current_and_carries_the_batch():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    assert "pub fn hk_deform_meshes(ctx: *mut HkCtx, items: *const HkMeshDeform, n: u32) -> i32;" in rust
    assert "pub fn hk_multi_deform_meshes(m: *mut HkMulti, items: *const HkMeshDeform, n: u32) -> i32;" in rust
    assert "size_of::<HkMeshDeform>() == 40" in rust


def test_abi_version_stays_8():
    assert F.api().abi_version() == 8
    assert re.search(r"#define\s+HK_ABI_VERSION\s+8u?\b", open(HEADER).read())


def test_null_context_is_refused_without_a_device():
    api = F.api()
    items = (F.HkMeshDeform * 1)()
    assert api.raw("deform_meshes")(None, items, 1) == F.HK_E_INVALID
    assert api.raw("deform_meshes")(None, None, 0) == F.HK_E_INVALID
    assert api.raw("multi_deform_meshes")(None, items, 1) == F.HK_E_INVALID
    assert api.raw("multi_deform_meshes")(None, None, 0) == F.HK_E_INVALID
    out = (F.u32 * 6)()
    assert api.raw("debug_last_deform")(None, out) == F.HK_E_INVALID


def test_library_exports_both_symbols():
    dll = F.api().dll
    for name in ("hk_deform_meshes", "hk_multi_deform_meshes", "hk_debug_last_deform"):
        assert hasattr(dll, name), name
    assert "hk_deform_meshes" in F.DECLARED_SYMBOLS and "hk_multi_deform_meshes" in F.DECLARED_SYMBOLS
    assert "hk_debug_last_deform" in F.DECLARED_DEBUG_SYMBOLS


def test_python_layers_offer_the_batch():
    """Engine, MultiEngine, BandRenderer and HikariPlugin each have deform_meshes; the item table keeps its arrays alive and refuses what it cannot name."""
    import numpy as np
    import pytest

    import bevy_hikari_amd as hk
    from bevy_hikari_amd import distributed as D
    from bevy_hikari_amd.plugin import deform_items

    for cls in (hk.Engine, hk.HikariPlugin, D.MultiEngine, D.BandRenderer):
        assert callable(getattr(cls, "deform_meshes", None)), cls
    assert callable(getattr(hk.Engine, "last_deform", None))
    mesh = F.HkMeshIndex(1, 2, 3, 4)
    pos = np.arange(12, dtype=np.float64).reshape(4, 3)
    table, keep = deform_items([("vertices", mesh, pos, None), ("skin", mesh, np.eye(4).reshape(1, 16)), ("vertices", mesh, pos, pos + 1)])
    assert (table[0].kind, table[0].count, bool(table[0].normals)) == (F.DEFORM_VERTICES, 4, False)
    assert (table[1].kind, table[1].count, bool(table[1].normals)) == (F.DEFORM_SKIN, 1, False)
    assert table[2].count == 4 and bool(table[2].normals) and table[2].mesh.node_count == 4
    assert [table[0].data[k] for k in range(12)] == list(range(12)) and table[2].normals[0] == 1.0
    with pytest.raises(ValueError):
        deform_items([("bones", mesh, pos)])
    with pytest.raises(ValueError):
        deform_items([("vertices", mesh, pos, pos[:2])])
