"""The overlay pass (hk_present, include/hikari_hip.h) restated in numpy, operation by operation, from the numeric contract's
primitives: np.float32 multiply / add / divide (IEEE, never fused), np.float16 for the f16 round trip, and the ORACLE's debug_math
for `pow_` (op 5) and the fma-chain `dot` (op 35) - the entry points tests/test_math_contract.py holds to the contract on the CPU.
Nothing here calls the library under test.

Planes are what `Engine.read` returns for an rgba16f buffer: uint16 [h][w][4].  `present` returns the target as the kernel leaves
it: uint8 [H][W][4] (the two 8-bit formats, bytes in memory order), float16 or float32 [H][W][4].

`make_planes` builds the adversarial source / albedo pair of the tests: one NaN in each of the four channels, each alone (one of
them over a NaN albedo), +-inf, negative values, +-0, an f16 denormal, 65504, alpha in {0, a denormal, 0.5, 1, 2}, a black texel
with alpha 1, and the values next to every sRGB code boundary."""
import math

import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import debug_math_call

f32 = np.float32
FORMATS = {"rgba16f": F.FORMAT_RGBA16F, "rgba32f": F.FORMAT_RGBA32F, "rgba8-srgb": F.FORMAT_RGBA8_UNORM_SRGB, "bgra8-srgb": F.FORMAT_BGRA8_UNORM_SRGB}
DTYPES = {"rgba16f": np.float16, "rgba32f": np.float32, "rgba8-srgb": np.uint8, "bgra8-srgb": np.uint8}
LUMA = (f32(0.2126), f32(0.7152), f32(0.0722))
H_NAN, H_INF, H_NINF, H_MAX, H_DENORMAL, H_NZERO = 0x7E00, 0x7C00, 0xFC00, 0x7BFF, 0x0001, 0x8000

# the material textures' sRGB -> linear table (scene_layout.hip): the EOTF in double, rounded to f32 once
SRGB_LUT = np.array([(v / 12.92 if v <= 0.04045 else math.pow((v + 0.055) / 1.055, 2.4)) for v in (i / 255.0 for i in range(256))], dtype=np.float32)


def _oracle():
    from oracle_lib import oracle_api

    return oracle_api()


def pow_(x, y):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return debug_math_call(_oracle(), None, 5, x.ravel(), np.full(x.size, y, dtype=np.float32)).reshape(x.shape)


def luminance(rgb):
    """dot(rgb, (0.2126, 0.7152, 0.0722)) as hk_device_math.hpp writes it: fma(z, c2, fma(y, c1, x * c0))"""
    q = np.zeros(rgb.shape[:-1] + (16,), dtype=np.float32)
    q[..., 0:3] = rgb
    q[..., 3:6] = LUMA
    return debug_math_call(_oracle(), None, 35, q.ravel()).reshape(rgb.shape[:-1])


def mix(a, b, t):
    return a * (f32(1.0) - t) + b * t


def sample(plane_u16, W, H):
    """The plane at every target pixel centre: the texel itself when the sizes agree, else sample_linear (kernels_aa.hip) at
    uv = ((x + 0.5) / W, (y + 0.5) / H), clamp-to-edge."""
    t = plane_u16.view(np.float16).astype(np.float32)
    h, w = t.shape[:2]
    if (w, h) == (W, H):
        return t

    def axis(n_out, n_in):
        uv = (np.arange(n_out, dtype=np.float32) + f32(0.5)) / f32(n_out)
        p = uv * f32(n_in) - f32(0.5)
        fl = np.floor(p)
        i = fl.astype(np.int64)
        return np.clip(i, 0, n_in - 1), np.clip(i + 1, 0, n_in - 1), (p - fl).astype(np.float32)

    x0, x1, fx = axis(W, w)
    y0, y1, fy = axis(H, h)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = mix(t[y0][:, x0], t[y0][:, x1], fx)
    bottom = mix(t[y1][:, x0], t[y1][:, x1], fx)
    return mix(top, bottom, fy)


def srgb_encode(v):
    return np.where(v <= f32(0.0031308), f32(12.92) * v, f32(1.055) * pow_(v, f32(1.0) / f32(2.4)) - f32(0.055)).astype(np.float32)


def unorm8_code(v):
    c = np.fmin(np.fmax(v, f32(0.0)), f32(1.0))         # clamp_ = fmin_(fmax_(x, lo), hi): a NaN becomes lo
    return np.floor(f32(0.5) + f32(255.0) * c).astype(np.uint8)


def decode(target, fmt):
    """the target's content as linear f32 rgba"""
    if fmt == "rgba16f":
        return target.astype(np.float32)
    if fmt == "rgba32f":
        return target.astype(np.float32, copy=True)
    rgb = target[..., 2::-1] if fmt == "bgra8-srgb" else target[..., :3]
    a8 = np.ascontiguousarray(target[..., 3], dtype=np.float32)
    alpha = debug_math_call(_oracle(), None, 20, a8.ravel()).reshape(a8.shape)                      # unorm8
    return np.concatenate([SRGB_LUT[rgb], alpha[..., None]], axis=-1)


def encode(o, fmt):
    if fmt == "rgba16f":
        return o.astype(np.float16)
    if fmt == "rgba32f":
        return o.astype(np.float32)
    rgb = unorm8_code(srgb_encode(o[..., :3]))
    if fmt == "bgra8-srgb":
        rgb = rgb[..., ::-1]
    return np.concatenate([rgb, unorm8_code(o[..., 3])[..., None]], axis=-1)


def blend_input(src_u16, albedo_u16, W, H, hdr):
    """steps 1-4: the colour the blend receives, f32 [H][W][4]"""
    with np.errstate(all="ignore"):
        c = sample(src_u16, W, H)
        bad = np.isnan(c).any(axis=-1)
        if bad.any():
            c = np.where(bad[..., None], sample(albedo_u16, W, H), c)
        if hdr:
            c = hdr_step(c)
    return c


def hdr_step(c):
    """inverse_reintard_luminance (overlay.wgsl) over bevy_core_pipeline 0.9.1's tonemapping_change_luminance"""
    with np.errstate(all="ignore"):
        lum = luminance(c[..., :3])
        l_old = np.fmin(np.fmax(lum, f32(0.0005)), f32(0.995))
        l_new = l_old / (f32(1.0) - l_old)
        s = (l_new / lum).astype(np.float32)
        return np.concatenate([c[..., :3] * s[..., None], c[..., 3:]], axis=-1).astype(np.float32)


def present(src_u16, albedo_u16, W, H, fmt, hdr=False, clear=None, target=None):
    """The target after hk_present: `clear` = four linear floats (HK_PRESENT_CLEAR), else `target` = its content before."""
    with np.errstate(all="ignore"):
        c = blend_input(src_u16, albedo_u16, W, H, hdr)
        d = np.broadcast_to(np.asarray(clear, dtype=np.float32), (H, W, 4)) if clear is not None else decode(target, fmt)
        a = c[..., 3:]
        k = f32(1.0) - a
        o = np.concatenate([c[..., :3] * a + d[..., :3] * k, a + d[..., 3:] * k], axis=-1).astype(np.float32)
        return encode(o, fmt)


def same(got, want):
    """byte for byte; in the float formats a NaN matches any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.uint8:
        return bool((got == want).all())
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    return bool(((got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))).all())


# ---------------------------------------------------------------------------------------------- adversarial planes
def srgb_boundaries():
    """the 255 linear values whose sRGB code changes there (255 * encode(v) = k + 0.5) and 1.0, as f16 bit patterns"""
    e = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    v = np.where(e <= 12.92 * 0.0031308, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)
    return np.concatenate([v, [1.0]]).astype(np.float16).view(np.uint16)


def f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def make_planes(src_size, albedo_size, seed=3):
    """-> (source, albedo) uint16 [h][w][4].  The special texels go to seeded places (the four corners among them, so that clamped
    bilinear footprints hold a NaN); a plane too small for all of them gets the first that fit - never the case at the test sizes."""
    rng = np.random.default_rng(seed)
    (w, h), (aw, ah) = src_size, albedo_size
    src = f16(rng.random((h, w, 4)) * 1.25)
    src[..., 3] = f16(rng.choice([0.0, 0.5, 1.0, 1.0, 1.0, 2.0], size=(h, w)))
    src[..., 3][rng.random((h, w)) < 0.05] = H_DENORMAL
    albedo = f16(0.1 + 0.8 * rng.random((ah, aw, 4)))
    albedo[..., 3] = f16(1.0)
    one, half = int(f16(1.0)), int(f16(0.5))
    b = srgb_boundaries()
    specials = [[H_NAN, half, half, one], [half, H_NAN, half, one], [half, half, H_NAN, half], [half, half, half, H_NAN],   # one NaN per channel, each alone
                [H_INF, half, half, one], [half, H_NINF, half, half], [H_INF, H_NINF, half, one],
                [int(f16(-0.25)), half, int(f16(-2.0)), one], [0, H_NZERO, 0, half], [H_NZERO, H_NZERO, H_NZERO, H_NZERO],
                [H_DENORMAL, H_DENORMAL, half, one], [H_DENORMAL, 0, 0, H_DENORMAL], [H_MAX, half, H_MAX, one], [H_MAX, H_MAX, H_MAX, H_MAX],
                [0, 0, 0, one],                                                                                            # black, alpha 1
                [half, half, half, 0], [half, half, half, H_DENORMAL], [half, half, half, int(f16(2.0))], [one, one, one, half]]
    corners = [0, w - 1, (h - 1) * w, h * w - 1]
    places = corners + [int(p) for p in rng.permutation(h * w) if p not in corners]
    flat = src.reshape(-1, 4)
    for texel, p in zip(specials, places):
        flat[p] = texel
    # the boundary values: one per texel (red for the first 86, then green, then blue), in raster order over the texels still free - neighbours one code apart,
    # so that a bilinear footprint over them is smooth (tests/test_present.py: the share of results a first-order bound cannot decide)
    free = sorted(set(range(h * w)) - set(places[:len(specials)]))[:256]
    for k, p in enumerate(free):
        texel = [int(f16(0.3 + 0.4 * k / 256.0)), int(f16(0.7 - 0.4 * k / 256.0)), int(f16(0.45)), one]
        texel[k // 86] = int(b[k])
        flat[p] = texel
    # the albedo under the first NaN texel (the top-left corner) holds a NaN too, and a few more wherever they fall
    albedo[0, 0] = [half, H_NAN, half, one]
    albedo.reshape(-1, 4)[rng.permutation(ah * aw)[:3]] = [H_NAN, half, H_INF, one]
    return src, albedo


def random_target(fmt, W, H, seed=11):
    """what a kept target holds before the present: every 8-bit code, finite floats and a few specials"""
    rng = np.random.default_rng(seed)
    if DTYPES[fmt] == np.uint8:
        return rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    t = (rng.random((H, W, 4)) * 2.0 - 0.5).astype(np.float32)
    flat = t.reshape(-1)
    flat[rng.permutation(flat.size)[:6]] = [np.nan, np.inf, -np.inf, -0.0, 65504.0, 6e-8]
    return t.astype(DTYPES[fmt])
