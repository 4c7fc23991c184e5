"""Textures from device memory (hk_update_textures_device, hk_read_texture, hk_encode_texels), the half that needs no GPU: the boundary
as every layer states it, and the host twin of the kernel's conversion against a numpy float32 restatement written here - products and
sums are np.float32 operations, each rounded on its own.  Every comparison is bit for bit."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import texture_source
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hikari_hip.h")
F32 = np.float32

# ---- the restatement: the sRGB decode table (the EOTF in double, rounded once), its 255 thresholds, the two rules
LUT = np.array([F32(v / 12.92 if v <= 0.04045 else math.pow((v + 0.055) / 1.055, 2.4)) for v in (i / 255.0 for i in range(256))], dtype=F32)
MID = np.array([F32(-1.0)] + [F32((float(LUT[k - 1]) + float(LUT[k])) / 2) for k in range(1, 256)], dtype=F32)


def clamp(x):
    x = np.asarray(x, dtype=F32)
    v = np.where(np.isnan(x), F32(0), x).astype(F32)
    return np.minimum(np.maximum(v, F32(0)), F32(1)).astype(F32)


def plain(x):
    p = (clamp(x) * F32(255.0)).astype(F32)        # one rounded product ...
    return (p + F32(0.5)).astype(F32).astype(np.uint32).astype(np.uint8)   # ... one rounded sum, truncated


def srgb(x):
    return (clamp(x)[..., None] > MID[1:]).sum(axis=-1).astype(np.uint8)   # the number of k in 1 .. 255 with v > mid[k]


def expected(values, linear=False, texture_srgb=True):
    """values: the logical [h][w][c] array (numpy has resolved the strides) -> uint8[h][w][4]"""
    values = values[..., None] if values.ndim == 2 else values
    h, w, c = values.shape
    out = np.zeros((h, w, 4), np.uint8)
    out[..., 3] = 255
    for ch in range(c):
        v = values[..., ch]
        if values.dtype == np.uint8:
            b = v
        else:
            b = srgb(v.astype(F32)) if linear and texture_srgb and ch < 3 else plain(v.astype(F32))
        out[..., ch] = b
    if c == 1:
        out[..., 1] = out[..., 2] = out[..., 0]
    return out


def logical(array, layout):
    return np.moveaxis(array, 0, 2) if array.ndim == 3 and layout == "chw" else array


def check(array, layout="hwc", **kw):
    got = hk.encode_texels(array, layout, **kw)
    want = expected(logical(array, layout), **kw)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]
    return got


def special_values():
    vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, -1e-30, 1.5, 2.0, 1e30, -1e30, 1e-45, -1e-45, 1e-40, 1.1754942e-38, 0.99999994, 1.0000001]
    for k in range(256):
        for centre in (k / 255.0, (k - 0.5) / 255.0, (k + 0.5) / 255.0):
            c = F32(centre)
            vals += [c, np.nextafter(c, F32(2)), np.nextafter(c, F32(-2)), np.nextafter(np.nextafter(c, F32(2)), F32(2)), np.nextafter(np.nextafter(c, F32(-2)), F32(-2))]
    return np.array(vals, dtype=F32)


# ---- the boundary
def test_header_ffi_and_library_agree_on_the_new_names():
    text = " ".join(re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S).split())
    assert "int hk_update_textures_device(hk_ctx* ctx, const HkTextureSource* items, uint32_t n, void* producer_stream);" in text
    assert "int hk_read_texture(hk_ctx* ctx, uint32_t index, uint8_t* rgba8, size_t bytes);" in text
    assert "int hk_encode_texels(const HkTextureSource* item, uint32_t texture_is_srgb, uint8_t* rgba8_out);" in text
    assert "hk_multi_update_textures_device" not in text   # a device pointer lives on one device
    for name, value in (("HK_TEXELS_U8", 0), ("HK_TEXELS_F16", 1), ("HK_TEXELS_F32", 2), ("HK_TEXTURE_SET_SAMPLER", 1), ("HK_TEXTURE_LINEAR_SOURCE", 2)):
        assert re.search(r"#define %s\s+%du\b" % (name, value), text), name
    assert (F.TEXELS_U8, F.TEXELS_F16, F.TEXELS_F32, F.TEXTURE_SET_SAMPLER, F.TEXTURE_LINEAR_SOURCE) == (0, 1, 2, 1, 2)
    assert F._PRODUCT_ONLY["update_textures_device"] == [C.c_void_p, C.POINTER(F.HkTextureSource), F.u32, C.c_void_p]
    assert F._PRODUCT_ONLY["read_texture"] == [C.c_void_p, F.u32, C.c_void_p, C.c_size_t]
    assert F._PRODUCT_ONLY["encode_texels"] == [C.POINTER(F.HkTextureSource), F.u32, C.c_void_p]
    for name in ("hk_update_textures_device", "hk_read_texture", "hk_encode_texels"):
        assert name in F.DECLARED_SYMBOLS and hasattr(F.api().dll, name), name
    assert "hk_debug_last_texture_update" in F.DECLARED_DEBUG_SYMBOLS and hasattr(F.api().dll, "hk_debug_last_texture_update")
    assert F.api().abi_version() == 8
    assert "NO CALL IS NEWLY REFUSED" in open(HEADER).read()


def test_the_struct_has_the_stated_size_and_offsets():
    S = F.HkTextureSource
    assert C.sizeof(S) == 80
    offsets = {name: getattr(S, name).offset for name, _ in S._fields_}
    assert offsets == dict(index=0, format=4, data=8, stride_x=16, stride_y=24, stride_c=32, channels=40, x0=44, y0=48, width=52, height=56, flags=60,
                           is_srgb=64, address_u=68, address_v=72, filter_linear=76)
    assert re.search(r"\}\s*HkTextureSource;\s*/\* 80 bytes", open(HEADER).read())


def test_generated_rust_crate_and_the_wrappers_carry_the_calls():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    assert "pub fn hk_update_textures_device(ctx: *mut HkCtx, items: *const HkTextureSource, n: u32, producer_stream: *mut c_void) -> i32;" in rust
    assert "pub fn hk_read_texture(ctx: *mut HkCtx, index: u32, rgba8: *mut u8, bytes: usize) -> i32;" in rust
    assert "pub fn hk_encode_texels(item: *const HkTextureSource, texture_is_srgb: u32, rgba8_out: *mut u8) -> i32;" in rust
    assert "assert!(core::mem::size_of::<HkTextureSource>() == 80)" in rust
    sig = inspect.signature(hk.Engine.update_textures)
    assert list(sig.parameters) == ["self", "items", "producer_stream"] and sig.parameters["producer_stream"].default is None
    assert list(inspect.signature(hk.HikariPlugin.update_textures).parameters) == list(sig.parameters)
    assert list(inspect.signature(hk.Engine.read_texture).parameters) == ["self", "index"]
    assert callable(getattr(hk.HikariPlugin, "read_texture", None))
    text = open(os.path.join(ROOT, "include", "hikari.hpp")).read()
    assert "hk_update_textures_device(" in text and "hk_read_texture(" in text


def test_host_texels_are_refused_with_a_type_error():
    engine = hk.Engine.__new__(hk.Engine)   # (no context: the check comes first)
    engine.device, engine._textures = 0, [dict(width=4, height=4, srgb=True, address_u=0, address_v=0, filter=True)]
    with pytest.raises(TypeError):
        hk.Engine.update_textures(engine, [dict(index=0, tensor=np.zeros((4, 4, 4), np.uint8))])


# ---- the conversion
@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_formats_channels_and_layouts(dtype, channels, layout):
    """a 7 x 5 rectangle; packed, as a column slice of a wider array, and with strides of zero"""
    rng = np.random.default_rng(channels * 7 + (layout == "chw"))
    shape = (5, 7, channels) if layout == "hwc" else (channels, 5, 7)
    wide = (5, 19, channels) if layout == "hwc" else (channels, 5, 19)

    def make(s):
        return rng.integers(0, 256, s, dtype=np.uint8) if dtype == np.uint8 else rng.uniform(-0.2, 1.2, s).astype(dtype)

    check(make(shape), layout)
    w = make(wide)
    check(w[:, 3:10, :] if layout == "hwc" else w[:, :, 3:10], layout)                    # a column slice: no copy
    row = make((1, 7, channels) if layout == "hwc" else (channels, 1, 7))
    check(np.broadcast_to(row, shape), layout)                                            # stride_y = 0
    one = make((5, 7, 1) if layout == "hwc" else (1, 5, 7))
    check(np.broadcast_to(one, shape), layout)                                            # stride_c = 0
    check(np.broadcast_to(make((1, 1, 1)), shape), layout)                                # every stride 0
    if channels == 1:
        check(make((5, 7)))                                                               # [h][w]: grey


def test_float_rule_on_special_values_and_every_boundary():
    vals = special_values()
    got = check(vals.reshape(1, -1))
    assert got[0, 0].tolist() == [0, 0, 0, 255] and got[0, 1].tolist() == [255, 255, 255, 255] and got[0, 2].tolist() == [0, 0, 0, 255]   # NaN, +Inf, -Inf
    check(np.stack([vals, vals[::-1], vals, vals[::-1]], axis=-1)[None])                  # ... and as rgba, alpha included
    k = np.arange(256)
    assert np.array_equal(hk.encode_texels((k / 255.0).astype(F32).reshape(1, -1))[0, :, 0], k)   # every k / 255 is byte k
    with np.errstate(over="ignore"):
        half = vals.astype(np.float16)   # (1e30 becomes Inf)
    check(half.reshape(1, -1))


def test_every_half_bit_pattern():
    halves = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(256, 256)
    check(halves)
    check(halves, linear=True)
    assert np.array_equal(hk.encode_texels(halves), hk.encode_texels(halves.astype(F32)))   # the widening is exact


def test_linear_source_inverts_the_decode_table():
    got = check(LUT.reshape(1, 256), linear=True)
    assert np.array_equal(got[0, :, 0], np.arange(256)) and (got[..., 3] == 255).all()     # encode(lut[b]) == b
    # every threshold and its two f32 neighbours land on the stated side: v > mid[k] counts k
    mid = MID[1:]
    at, above, below = (hk.encode_texels(a.reshape(1, -1), linear=True)[0, :, 0] for a in (mid, np.nextafter(mid, F32(2)), np.nextafter(mid, F32(-2))))
    k = np.arange(1, 256)
    assert np.array_equal(at, k - 1) and np.array_equal(above, k) and np.array_equal(below, k - 1)
    check(special_values().reshape(1, -1), linear=True)
    sample = np.sort(np.random.default_rng(5).uniform(-0.1, 1.1, 20000).astype(F32))
    out = check(sample.reshape(100, 200), linear=True)[..., 0].reshape(-1).astype(int)
    assert (np.diff(out) >= 0).all() and out[0] == 0 and out[-1] == 255                    # monotone


def test_linear_source_leaves_alpha_and_other_textures_to_the_plain_rule():
    rng = np.random.default_rng(6)
    rgba = rng.uniform(-0.1, 1.1, (5, 7, 4)).astype(F32)
    enc = check(rgba, linear=True, texture_srgb=True)
    assert np.array_equal(enc[..., 3], plain(rgba[..., 3])) and np.array_equal(enc[..., :3], srgb(rgba[..., :3]))
    assert not np.array_equal(enc[..., :3], plain(rgba[..., :3]))
    flat = check(rgba, linear=True, texture_srgb=False)                                   # not an sRGB texture: every channel plain
    assert np.array_equal(flat, hk.encode_texels(rgba))
    check(rgba.astype(np.float16), "hwc", linear=True)
    check(np.ascontiguousarray(np.moveaxis(rgba, 2, 0)), "chw", linear=True)


# ---- refusals that need no device
def test_refusals_of_the_encoder_and_of_the_context_calls():
    api = F.api()
    encode = api.raw("encode_texels")
    out = np.zeros((5, 7, 4), np.uint8)
    pixels = np.zeros((5, 7, 4), F32)

    def item(**kw):
        s = texture_source(0, kw.pop("array", pixels))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    assert encode(C.byref(item()), 1, out.ctypes.data) == F.HK_OK
    bad = dict(format=item(format=3), flag=item(flags=4), channels=item(channels=2), no_channels=item(channels=0),
               linear_u8=item(array=np.zeros((5, 7, 4), np.uint8), flags=F.TEXTURE_LINEAR_SOURCE), no_data=item(data=None),
               empty_width=item(width=0), empty_height=item(height=0), stride_x=item(stride_x=18), stride_y=item(stride_y=114), stride_c=item(stride_c=2),
               half_stride=item(array=np.zeros((5, 7, 4), np.float16), stride_x=9), pointer=item(data=pixels.ctypes.data + 2))
    for name, it in bad.items():
        assert encode(C.byref(it), 1, out.ctypes.data) == F.HK_E_INVALID, name
        assert api.last_error(), name
    assert encode(None, 1, out.ctypes.data) == F.HK_E_INVALID and encode(C.byref(item()), 1, None) == F.HK_E_INVALID
    assert not out.any()                                                                   # a refused call writes nothing
    table = (F.HkTextureSource * 1)(item())
    assert api.raw("update_textures_device")(None, table, 1, None) == F.HK_E_INVALID
    assert api.raw("update_textures_device")(None, None, 0, None) == F.HK_E_INVALID
    assert "NULL" in api.last_error()
    assert api.raw("read_texture")(None, 0, out.ctypes.data, out.size) == F.HK_E_INVALID
    assert api.raw("debug_last_texture_update")(None, None) == F.HK_E_INVALID
