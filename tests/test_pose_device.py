"""The boundary of instance poses from device memory (hk_set_instance_transforms_device, hk_read_instance_transforms) as every layer
states it - header, ctypes table, generated Rust crate, C++ and Python wrappers - and what the two entry points answer without a device."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hikari_hip.h")


def header_text():
    return " ".join(re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S).split())


def test_header_declares_both_functions():
    text = header_text()
    assert ("int hk_set_instance_transforms_device(hk_ctx* ctx, hk_scene_builder* b, const uint32_t* instance_ids, uint32_t n, const void* d_models, "
            "uint32_t stride_bytes, void* producer_stream, uint32_t* d_status);") in text
    assert "int hk_read_instance_transforms(hk_ctx* ctx, float* models, uint32_t n);" in text
    assert "hk_multi_set_instance_transforms_device" not in text   # a device pointer lives on one device: no multi form
    comment = open(HEADER).read()
    assert "no hk_multi_ form" in comment


def test_ctypes_table_carries_both_calls():
    assert F._PRODUCT_ONLY["set_instance_transforms_device"] == [C.c_void_p, C.c_void_p, C.POINTER(F.u32), F.u32, C.c_void_p, F.u32, C.c_void_p, C.c_void_p]
    assert F._PRODUCT_ONLY["read_instance_transforms"] == [C.c_void_p, C.POINTER(F.f32), F.u32]
    for name in ("hk_set_instance_transforms_device", "hk_read_instance_transforms"):
        assert name in F.DECLARED_SYMBOLS
        assert hasattr(F.api().dll, name), name
    assert "hk_debug_last_pose" in F.DECLARED_DEBUG_SYMBOLS and hasattr(F.api().dll, "hk_debug_last_pose")


def test_generated_rust_crate_is_current_and_carries_the_calls():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    assert ("pub fn hk_set_instance_transforms_device(ctx: *mut HkCtx, b: *mut HkSceneBuilder, instance_ids: *const u32, n: u32, d_models: *const c_void, "
            "stride_bytes: u32, producer_stream: *mut c_void, d_status: *mut u32) -> i32;") in rust
    assert "pub fn hk_read_instance_transforms(ctx: *mut HkCtx, models: *mut f32, n: u32) -> i32;" in rust


def test_abi_version_stays_8_and_the_entry_points_answer_without_a_device():
    api = F.api()
    assert api.abi_version() == 8
    b = hk.SceneBuilder()
    ids = (F.u32 * 1)(0)
    models = (F.f32 * 16)()
    call = api.raw("set_instance_transforms_device")
    assert call(None, b.h, ids, 1, C.addressof(models), 64, None, None) == F.HK_E_INVALID
    assert call(None, None, None, 0, None, 64, None, None) == F.HK_E_INVALID
    assert "NULL" in api.last_error()
    assert api.raw("read_instance_transforms")(None, models, 1) == F.HK_E_INVALID
    assert api.raw("read_instance_transforms")(None, None, 0) == F.HK_E_INVALID
    assert api.raw("debug_last_pose")(None, None) == F.HK_E_INVALID


def test_python_and_cpp_layers_offer_the_call():
    sig = inspect.signature(hk.Engine.set_instance_transforms)
    assert list(sig.parameters) == ["self", "builder", "models", "ids", "producer_stream", "status"]
    assert [sig.parameters[k].default for k in ("ids", "producer_stream", "status")] == [None, None, None]
    assert callable(getattr(hk.Engine, "read_instance_transforms", None))
    assert list(inspect.signature(hk.HikariPlugin.set_instance_transforms).parameters) == list(sig.parameters)
    assert callable(getattr(hk.HikariPlugin, "read_instance_transforms", None))
    text = open(os.path.join(ROOT, "include", "hikari.hpp")).read()
    assert "hk_set_instance_transforms_device(" in text and "hk_read_instance_transforms(" in text


def test_host_poses_are_refused_with_a_type_error():
    """A numpy array (or a torch tensor on the host) is not what this path is for: TypeError before any context is touched."""
    import numpy as np
    import pytest

    engine = hk.Engine.__new__(hk.Engine)   # (no context: the check comes first)
    engine.device = 0
    with pytest.raises(TypeError):
        hk.Engine.set_instance_transforms(engine, hk.SceneBuilder(), np.zeros((2, 16), np.float32))
    try:
        import torch
    except ImportError:
        return
    with pytest.raises(TypeError):
        hk.Engine.set_instance_transforms(engine, hk.SceneBuilder(), torch.zeros((2, 4, 4)))
