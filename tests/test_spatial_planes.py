"""The oracle's spatial_reuse (light.wgsl:1500-1684, both pipelines) on the adversarial planes of tests/post_planes.py
(`make_spatial_planes`), held three ways: against a float64 restatement of the shader, against what the reference's own shader wrote
on the planes (tests/golden/wgsl_spatial_planes_*.npz), and - in tests/test_spatial_planes_gpu.py - the kernels against the oracle bit
for bit.

The restatement is written from the shader's text and bevy_pbr 0.9.1's published lighting functions, every pixel at once.  What is exact
in f32 is replayed in f32: the tap's radius, interval, step count and j / (n + 1), the turn count i * golden + dot(random, 1) +
random_float(frame) and fract(dot(random, 1)), the deferred texel of a pixel centre and the march comparison.  Every other decision is
taken in float64 and noted in a `margin` mask where its operands lie within rounding of the threshold (by reason: `Restated.reasons`);
`open` marks normalize(0).  Per pixel it also returns the branch counts: the five reject reasons the kernel's HK_TAP statistics name,
merges that replace the sample and that keep it, history taken / refused / outside, the clamp, the variance store, the background
re-pack, the step a march ends at.

Bounded on `terraces` alone, over every shape of SPATIAL_WIDTHS x SPATIAL_HEIGHTS, ratio, parity and limit, both channels: `render` and
the four statistics in f16 ulps, the variance in f32 ulps of the MINUEND w2_sum / count (the subtraction cancels), the picked
radiance, the stored visible position and the lifetime byte identical.  BOUNDS are twice the worst deviation measured, next whole ulp
(DESIGN.md section 2).  At most 2 % of a dispatch's geometry pixels may be left out (below 585 pixels: rounded up to a whole pixel), and
no placed pixel of `terraces`.  Planted mistakes must fail."""
import os

import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F
from test_post_chain_planes import deviation_f16, half


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import oracle_plugin

    p = oracle_plugin()
    p.set_scene(PP.spatial_scene())
    return p.engine


# ---------------------------------------------------------------- the packer
def test_pack_records_is_a_fixed_point_of_the_oracles_unpack_and_pack():
    """`pack_records` against orc_kat_reservoir_roundtrip (unpack_reservoir, then pack_reservoir: light.wgsl:77-136): every word but the
    re-normalised normals comes back as packed, the lifetime and flag bytes included; the normals keep their direction."""
    from oracle_lib import oracle_api

    p = PP.make_spatial_planes("terraces", 7, (17, 17), 1.0, 2, 2)
    r = p.current
    r.lifetime[0, :5] = (0, 1, 126, 127, 254)
    packed = PP.pack_records(r).reshape(-1, 16)
    keep = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 15]
    for rec, life, flag in zip(packed, r.lifetime.reshape(-1), r.jacobian_flag.reshape(-1)):
        rec, out = np.ascontiguousarray(rec), np.zeros(16, np.uint32)
        oracle_api().dll.orc_kat_reservoir_roundtrip(rec.ctypes.data, out.ctypes.data)
        assert (out[keep] == rec[keep]).all()
        a, b = out[12:14].view(np.int8).reshape(2, 4), rec[12:14].view(np.int8).reshape(2, 4)
        assert (a[:, 3] == b[:, 3]).all() and int(b[0, 3]) == int(life) - 127 and int(b[1, 3]) == int(flag)
        for i in range(2):
            va, vb = a[i, :3].astype(float), b[i, :3].astype(float)
            assert np.dot(va, vb) / (np.linalg.norm(va) * np.linalg.norm(vb)) > 0.9995
    # the fields where the layout says they are: count and w in word 14, w_sum and w2_sum in word 15, the instance in word 11
    assert (packed[:, 14] & 0xFFFF == r.count.reshape(-1)).all() and (packed[:, 15] >> 16 == r.w2_sum.reshape(-1)).all()
    assert (packed[:, 11].view(np.float32) == r.visible_instance.reshape(-1)).all()


def test_the_top_of_the_history_range_stays_inside_the_buffer():
    """previous_uv one ulp under 1 (the `history` set): i32(uv * size) is at most size - 1, because size * (1 - 2^-24) never rounds up to
    size in f32 - asserted here for every tested width and height rather than by reading memory"""
    under_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    for n in sorted(set(PP.SPATIAL_WIDTHS) | set(PP.SPATIAL_HEIGHTS) | {24, 16}):
        assert int(np.float32(under_one * np.float32(n))) == n - 1
    for ratio in PP.SPATIAL_RATIOS:
        for parity in (2, 3):
            p = PP.make_spatial_planes("history", 7, (70, 45), ratio, 2, parity)
            assert np.isnan(p.buffers[F.BUF_VELOCITY_UV][..., :2]).any() and np.isinf(p.buffers[F.BUF_VELOCITY_UV][..., :2]).any()


def test_the_quarter_turn_search_still_finds_its_codes():
    """the `records` set: per quarter turn the unorm16 code that brings some tap's angle nearest to it - closer than 2^-16 of a turn"""
    for frame_number in (2, 3):
        for count in (8, 16):
            for target, (code, i) in zip((0.0, 0.25, 0.5, 0.75), PP.quarter_turn_randoms(frame_number, count)):
                t = np.float32(np.float32(np.float32(i) * np.float32(1.618033989)) + np.float32(code) / np.float32(65535.0)) + PP.random_float(frame_number)
                fr = float(np.float32(t - np.floor(t)))
                assert min(abs(fr - target), abs(fr - target - 1.0)) < 2.0 ** -16


# ---------------------------------------------------------------- spatial_reuse in float64, from light.wgsl:1500-1684
F32 = lambda v: float(np.float32(v))
GOLDEN_RATIO, TAU, F32_EPSILON, F32_MAX = F32(1.618033989), F32(6.283185307), F32(1.1920929e-7), F32(3.402823466e38)
PI = F32(3.141592653589793)                          # bevy_pbr 0.9.1 utils.wgsl
LUMA = np.array([F32(0.2126), F32(0.7152), F32(0.0722)])
REJECTS = ("outside", "depth_ratio", "empty_or_normal", "facing_away", "occluded")        # the kernel's HK_TAP statistics 1 .. 5
MISTAKES = ("march_ge", "normal_09", "no_jacobian", "no_clamp", "visible_not_restored", "eight_taps", "tests_after_weight", "variance_always_divided")


def dot(a, b):
    return (a * b).sum(axis=-1)


def normalize(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt(dot(v, v))[..., None]


def luminance(c):
    return dot(c[..., :3], LUMA)


def saturate(v):
    return np.clip(v, 0.0, 1.0)


def unpack(records):
    """unpack_reservoir (light.wgsl:77-109) of a Records grid, in float64"""
    r = {"count": half(records.count), "w": half(records.w), "w_sum": half(records.w_sum), "w2_sum": half(records.w2_sum),
         "radiance": half(records.radiance), "random": records.random.astype(np.float64) / 65535.0,
         "visible_position": records.visible_position.astype(np.float64), "sample_position": records.sample_position.astype(np.float64),
         "visible_normal": normalize(np.maximum(records.visible_normal.astype(np.float64) / 127.0, -1.0)),
         "sample_normal": normalize(np.maximum(records.sample_normal.astype(np.float64) / 127.0, -1.0)),
         "flag": np.maximum(records.jacobian_flag.astype(np.float64) / 127.0, -1.0),
         "lifetime": 127.0 * (1.0 + np.maximum((records.lifetime.astype(np.float64) - 127.0) / 127.0, -1.0)),
         "radiance_bits": records.radiance.copy(), "random32": records.random.astype(np.float32) / np.float32(65535.0)}
    return r


SAMPLE_FIELDS = ("radiance", "random", "random32", "sample_position", "sample_normal", "flag", "radiance_bits", "visible_position", "visible_normal")


def take(r, rows, cols):
    return {k: v[rows, cols] for k, v in r.items()}


def shading(V, N, L, surface, radiance, ambient_color):
    """shading / lit / ambient (light.wgsl:796-888) over bevy_pbr 0.9.1's pbr_lighting.wgsl"""
    with np.errstate(all="ignore"):
        base, metallic, roughness, reflectance = surface["base_color"], surface["metallic"][..., None], surface["roughness"], surface["reflectance"][..., None]
        F0 = F32(0.16) * reflectance * reflectance * (1.0 - metallic) + base * metallic
        diffuse_color = base * (1.0 - metallic)
        H = normalize(L + V)
        NoL, NoH, LoH = saturate(dot(N, L)), saturate(dot(N, H)), saturate(dot(L, H))
        NdotV = np.maximum(dot(N, V), F32(0.0001))
        schlick = lambda f0, f90, VoH: f0 + (f90 - f0) * (1.0 - VoH) ** 5
        f90 = F32(0.5) + 2.0 * roughness * LoH * LoH                                                    # Fd_Burley
        burley = schlick(1.0, f90, NoL) * schlick(1.0, f90, NdotV) * (1.0 / PI)
        a = NoH * roughness                                                                             # D_GGX
        k = roughness / (1.0 - NoH * NoH + a * a)
        D = k * k * (1.0 / PI)
        a2 = roughness * roughness                                                                      # V_SmithGGXCorrelated
        Vis = F32(0.5) / (NoL * np.sqrt((NdotV - a2 * NdotV) * NdotV + a2) + NdotV * np.sqrt((NoL - a2 * NoL) * NoL + a2))
        f90s = saturate(dot(F0, np.full(3, F32(50.0) * F32(0.33))))                                      # fresnel
        Fr = F0 + (f90s[..., None] - F0) * ((1.0 - LoH) ** 5)[..., None]
        specular = (D * Vis)[..., None] * Fr
        lit = (specular + diffuse_color * burley[..., None]) * radiance[..., :3] * NoL[..., None]

        def env(f0, perceptual_roughness):                                                              # EnvBRDFApprox
            c0, c1 = np.array([-1.0, F32(-0.0275), F32(-0.572), F32(0.022)]), np.array([1.0, F32(0.0425), F32(1.04), F32(-0.04)])
            rr = perceptual_roughness[..., None] * c0 + c1
            a004 = np.minimum(rr[..., 0] * rr[..., 0], np.exp2(F32(-9.28) * NdotV)) * rr[..., 0] + rr[..., 1]
            return f0 * (F32(-1.04) * a004 + rr[..., 2])[..., None] + (F32(1.04) * a004 + rr[..., 3])[..., None]

        ambient = surface["occlusion"] * (env(diffuse_color, np.ones_like(roughness)) + env(F0, roughness)) * ambient_color
        t = (1.0 - radiance[..., 3])[..., None]
        return lit * (1.0 - t) + ambient * t


class Restated:
    pass


def restate(planes, mistake=None):
    """spatial_reuse of light.wgsl on the planes, every pixel at once.  Decisions whose operands are exact in f32 - the march comparison,
    the tap's radius, interval and step count - are replayed in f32; every other decision is taken in float64 and noted in `margin`
    where its operands lie within rounding of the threshold.  `open` marks what WGSL leaves open: normalize(0)."""
    assert mistake is None or mistake in MISTAKES
    f = planes.frame
    (dw, dh), (rw, rh), emissive = planes.window_size, planes.render_size, planes.channel == 1
    n_taps, reach = (8, 10.0) if emissive else (16, 20.0)
    if mistake == "eight_taps":
        n_taps = 8 if not emissive else 4
    position = planes.buffers[F.BUF_POSITION].astype(np.float64)
    depth32 = np.ascontiguousarray(planes.buffers[F.BUF_POSITION][..., 3])
    material = planes.buffers[F.BUF_INSTANCE_MATERIAL][..., 1]
    velocity = planes.buffers[F.BUF_VELOCITY_UV].astype(np.float64)
    cur, hist = unpack(planes.current), unpack(planes.previous_spatial)
    ys, xs = np.meshgrid(np.arange(rh), np.arange(rw), indexing="ij")
    margin, open_, reasons = np.zeros((rh, rw), bool), np.zeros((rh, rw), bool), {}

    def note(reason, mask):
        margin[...] |= mask
        reasons[reason] = reasons.get(reason, np.zeros((rh, rw), bool)) | mask
    sgn = -0.25 if f.number % 2 == 0 else 0.25
    jitter = np.array([sgn * F32(np.float32(1.0) / np.float32(dw)), sgn * F32(np.float32(1.0) / np.float32(dh))]) * (F32(f.upscale_ratio) - 1.0)

    def deferred(u, v):
        """jittered_deferred_coords: (row, column, inside the plane, the depth there as f32, `close`: within 5e-5 of a texel boundary
        across which the depth differs)"""
        with np.errstate(all="ignore"):
            px, py = (u + jitter[0]) * dw, (v + jitter[1]) * dh

            def fetch(px_, py_):
                cx, cy = np.trunc(px_), np.trunc(py_)
                ok = (cx >= 0) & (cy >= 0) & (cx < dw) & (cy < dh) & (px_ > -1.0) & (py_ > -1.0)
                ix, iy = np.clip(cx, 0, dw - 1).astype(np.int64), np.clip(cy, 0, dh - 1).astype(np.int64)
                return iy, ix, ok, np.where(ok, depth32[iy, ix], np.float32(0.0))

            iy, ix, ok, d = fetch(px, py)
            close = np.zeros(px.shape, bool)
            for ox in (-5e-5, 5e-5):
                for oy in (-5e-5, 5e-5):
                    alt = fetch(px + ox, py + oy)[3]
                    close |= alt.view(np.uint32) != d.view(np.uint32)
        return iy, ix, ok, d, close

    def deferred_of_pixel(px_x, px_y):
        """jittered_deferred_coords(coords_to_uv(pixel)) replayed in f32: divide, multiply and add on exact operands, nothing to round
        differently (at some sizes a whole column lands EXACTLY on a texel boundary)"""
        one = np.float32(1.0)
        s32, ratio32 = np.float32(sgn), np.float32(np.float32(f.upscale_ratio) - one)
        ju = (px_x.astype(np.float32) + np.float32(0.5)) / np.float32(rw) + (s32 * (one / np.float32(dw))) * ratio32
        jv = (px_y.astype(np.float32) + np.float32(0.5)) / np.float32(rh) + (s32 * (one / np.float32(dh))) * ratio32
        tx, ty = np.trunc(ju * np.float32(dw)).astype(np.int64), np.trunc(jv * np.float32(dh)).astype(np.int64)
        ok = (tx >= 0) & (ty >= 0) & (tx < dw) & (ty < dh)
        iy, ix = np.clip(ty, 0, dh - 1), np.clip(tx, 0, dw - 1)
        return iy, ix, np.where(ok, depth32[iy, ix], np.float32(0.0))

    u, v = (xs + 0.5) / rw, (ys + 0.5) / rh
    cy, cx, depth = deferred_of_pixel(xs, ys)
    out = Restated()
    with np.errstate(all="ignore"):
        out.background = background = depth < np.float32(F32_EPSILON)
    geometry = ~background
    # ---- the pixel's own reservoir, the surface, the history
    s = cur
    mid = np.clip(np.nan_to_num(material[cy, cx]), 0, len(PP.SPATIAL_MATERIALS) - 1).astype(np.int64)
    table = PP.SPATIAL_MATERIALS
    clamp_rough = lambda p: np.clip(F32(p), F32(0.089), 1.0) ** 2                                         # perceptualRoughnessToRoughness
    surface = {"base_color": np.array([[F32(c) for c in m[0]] for m in table])[mid], "metallic": np.array([F32(m[1]) for m in table])[mid],
               "roughness": np.array([clamp_rough(m[2]) for m in table])[mid], "reflectance": np.array([F32(0.3 + 0.1 * k) for k in range(len(table))])[mid],
               "occlusion": 1.0}
    lights, camera = hk.lights_uniform(), hk.cornell_camera(*planes.window_size).view_uniform()
    ambient_color = np.array([F32(lights.ambient_color[i]) for i in range(3)])
    V = normalize(np.array([F32(camera.world_position[i]) for i in range(3)]) - position[cy, cx, :3])
    N = s["visible_normal"]
    open_ |= np.isnan(N).any(axis=-1) & geometry
    shade = lambda L, radiance: shading(V, N, L, surface, radiance, ambient_color)
    with np.errstate(all="ignore"):
        use_variance = s["count"] <= 4.0
        limit = F32_MAX if F32(f.max_reservoir_lifetime) <= 1.0 else F32(f.max_reservoir_lifetime)
        wants_history = s["lifetime"] <= limit
        note("lifetime at the limit", geometry & (np.abs(s["lifetime"] - limit) < 1e-3))
        pu, pv = u + jitter[0] - velocity[cy, cx, 0], v + jitter[1] - velocity[cy, cx, 1]
        on_screen = (np.abs(pu - 0.5) < 0.5) & (np.abs(pv - 0.5) < 0.5)
        note("history uv at 0 or 1", geometry & wants_history & ((np.abs(np.abs(pu - 0.5) - 0.5) < 1e-6) | (np.abs(np.abs(pv - 0.5) - 0.5) < 1e-6)))
        hx, hy = np.where(on_screen, pu * rw, 0.0), np.where(on_screen, pv * rh, 0.0)
        note("history pixel boundary", geometry & wants_history & on_screen & ((np.abs(hx - np.rint(hx)) < 1e-4) | (np.abs(hy - np.rint(hy)) < 1e-4)))
        hy_i, hx_i = np.clip(np.trunc(hy), 0, rh - 1).astype(np.int64), np.clip(np.trunc(hx), 0, rw - 1).astype(np.int64)
    out.history_taken = taken = wants_history & on_screen & geometry
    out.history_refused = geometry & ~wants_history
    out.history_outside = geometry & wants_history & ~on_screen
    r = {k: np.where(taken.reshape(taken.shape + (1,) * (cur[k].ndim - 2)), hist[k][hy_i, hx_i], np.where((wants_history & ~on_screen).reshape(taken.shape + (1,) * (cur[k].ndim - 2)), 0.0, cur[k]).astype(cur[k].dtype))
         for k in cur}
    source = np.where(taken, -2, np.where(wants_history, -3, -1))          # whose sample the reservoir holds: -3 none (a zero record), -2 the history's, -1 the pixel's own, i a tap's
    out.merges, out.replaced, out.kept = np.zeros((rh, rw), int), np.zeros((rh, rw), int), np.zeros((rh, rw), int)
    out.rejects = {k: np.zeros((rh, rw), int) for k in REJECTS}
    out.march_end = {j: np.zeros((rh, rw), int) for j in range(1, 6)}

    def merge(r, source, q, p, active, code):
        """merge_reservoir + update_reservoir (light.wgsl:146-179) where `active`"""
        with np.errstate(all="ignore"):
            w_new = p * q["w"] * q["count"]
            w_sum = r["w_sum"] + w_new
            c32 = q["random32"]
            rand_sum = ((c32[..., 0] + c32[..., 1]) + c32[..., 2]) + c32[..., 3]          # fract(dot(random, 1)) as f32 forms it
            rand = (rand_sum - np.floor(rand_sum)).astype(np.float64)
            ratio = w_new / w_sum
            pick = rand < ratio
            near = np.abs(rand - ratio) < 3e-5
        note("random pick", active & near & geometry)
        for k in ("w_sum", "w2_sum", "count"):
            new = {"w_sum": w_sum, "w2_sum": r["w2_sum"] + w_new * w_new, "count": r["count"] + q["count"]}[k]
            r[k] = np.where(active, new, r[k])
        take_it = active & pick
        for k in SAMPLE_FIELDS:
            r[k] = np.where(take_it.reshape(take_it.shape + (1,) * (r[k].ndim - 2)), q[k], r[k])
        return np.where(take_it, code, source), take_it

    with np.errstate(all="ignore"):
        own_p = luminance(s["radiance"]) if emissive else luminance(shade(normalize(s["sample_position"] - s["visible_position"][..., :3]), s["radiance"]))
        open_ |= geometry & np.isnan(normalize(s["sample_position"] - s["visible_position"][..., :3])).any(axis=-1)
    source, _ = merge(r, source, s, own_p, geometry, -1)
    if mistake != "visible_not_restored":
        r["visible_position"], r["visible_normal"] = s["visible_position"].copy(), s["visible_normal"].copy()
    # the tap's angle in f32, operation for operation (exact IEEE multiply, add, floor): in float64 it would sit up to 3e-4 pixels off the
    # shader's own at radius 20, f32 rounding the turn count at 2e-6
    codes = planes.current.random.astype(np.float32) / np.float32(65535.0)
    rot32 = ((codes[..., 0] + codes[..., 1]) + codes[..., 2]) + codes[..., 3]
    rf32 = PP.random_float(int(f.number))
    for i in range(1, n_taps + 1):
        # the tap's own constants: exact IEEE operations of f32, replayed as such
        radius32 = np.float32(np.sqrt(np.float32(np.float32(i) / np.float32(8 if emissive else 16))) * np.float32(reach))
        interval32 = max(np.float32(1.0), np.float32(radius32 / np.float32(5.0)))
        steps = int(np.float32(radius32 / interval32))
        with np.errstate(all="ignore"):
            turn32 = (np.float32(np.float32(i) * np.float32(GOLDEN_RATIO)) + rot32) + rf32
            angle = (np.float32(TAU) * (turn32 - np.floor(turn32))).astype(np.float64)
            ox, oy = float(radius32) * np.cos(angle), float(radius32) * np.sin(angle)
            fx, fy = ox + xs, oy + ys
            near_int = lambda t: (np.abs(t - np.rint(t)) < 8e-6) & (np.rint(t) != 0.0)
            tap_margin = (near_int(fx) | near_int(fy)) & (fx > -1.001) & (fy > -1.001) & (fx < rw + 0.001) & (fy < rh + 0.001)      # (outside the image either way: no decision hangs on it)
            sx, sy = np.trunc(fx), np.trunc(fy)
            inside = (sx >= 0) & (sy >= 0) & (sx < rw) & (sy < rh)
            sx_i, sy_i = np.clip(sx, 0, rw - 1).astype(np.int64), np.clip(sy, 0, rh - 1).astype(np.int64)
            _, _, sample_depth = deferred_of_pixel(sx_i, sy_i)
            q = take(cur, sy_i, sx_i)
            alive = geometry.copy()
            note("tap pixel boundary", alive & tap_margin)
            why = {}
            why["outside"] = alive & ~inside
            alive &= inside
            ratio = depth.astype(np.float64) / sample_depth.astype(np.float64)
            ratio_miss = (ratio < F32(0.9)) | (ratio > F32(1.1))
            note("depth ratio", alive & ((np.abs(ratio - F32(0.9)) < 1e-6) | (np.abs(ratio - F32(1.1)) < 1e-6)))
            ndot = dot(N, q["visible_normal"])
            threshold = F32(0.9) if mistake == "normal_09" else F32(0.866)
            record_miss = (q["count"] < F32_EPSILON) | (ndot < threshold)
            to_sample = q["sample_position"] - s["visible_position"][..., :3]
            direction = normalize(to_sample)
            facing = dot(direction, N)
            away = facing < 0.0
            late_tests = mistake == "tests_after_weight"
            why["depth_ratio"] = alive & ratio_miss
            alive &= ~ratio_miss
            if not late_tests:
                note("normal threshold", alive & (np.abs(ndot - threshold) < 1e-5))
                why["empty_or_normal"] = alive & record_miss
                alive &= ~record_miss
                open_ |= alive & np.isnan(direction).any(axis=-1)
                note("facing", alive & (np.abs(facing) < 1e-6))
                why["facing_away"] = alive & away
                alive &= ~away
            # the march, with its break: the comparison replayed in f32 on exact operands
            occluded = np.zeros((rh, rw), bool)
            length = np.sqrt(ox * ox + oy * oy)
            for j in range(1, steps + 1):
                dist = float(np.float32(np.float32(j) * interval32))
                t32 = np.float32(np.float32(j) / np.float32(steps + 1))
                _, _, _, tap_depth, close = deferred(u + dist * (ox / length) / rw, v + dist * (oy / length) / rh)
                ref32 = (depth * np.float32(np.float32(1.0) - t32)).astype(np.float32) + (sample_depth * t32).astype(np.float32)
                bound = ref32.astype(np.float32) + np.float32(0.00001)
                hit = (tap_depth >= bound) if mistake == "march_ge" else (tap_depth > bound)
                first = alive & ~occluded & hit
                note("march texel boundary", alive & ~occluded & close)
                out.march_end[min(j, 5)] += first
                occluded |= first
            why["occluded"] = alive & occluded
            alive &= ~occluded
            jacobian = np.ones((rh, rw))
            if mistake != "no_jacobian":
                normal = q["sample_normal"]
                a = s["visible_position"][..., :3]
                cos_1 = np.abs(dot(normalize(a - q["sample_position"]), normal))
                cos_2 = np.abs(dot(normalize(q["visible_position"][..., :3] - q["sample_position"]), normal))
                num = dot(q["visible_position"][..., :3] - q["sample_position"], q["visible_position"][..., :3] - q["sample_position"])
                den = dot(a - q["sample_position"], a - q["sample_position"])
                jac = np.clip(cos_1 / np.maximum(F32(0.0001), cos_2) * (num / np.maximum(den, F32(0.0001))), 1.0, 50.0)
                jacobian = np.where(q["flag"] > 0.5, jac, 1.0)
            p = (luminance(q["radiance"]) if emissive else luminance(shade(direction, q["radiance"]))) / jacobian
        for k in REJECTS:
            out.rejects[k] += why.get(k, np.zeros((rh, rw), bool))
        source, took = merge(r, source, q, p, alive, i)
        out.merges += alive
        out.replaced += took
        out.kept += alive & ~took
    with np.errstate(all="ignore"):
        m = float(f.max_spatial_reuse_count)
        out.clamped = clamped = geometry & (r["count"] > m) & (mistake != "no_clamp")
        scale = np.where(clamped, m / r["count"], 1.0)
        r["w_sum"], r["w2_sum"], r["count"] = r["w_sum"] * scale, r["w2_sum"] * scale, np.where(clamped, m, r["count"])
        out_radiance = shade(normalize(r["sample_position"] - s["visible_position"][..., :3]), r["radiance"])
        total_lum = r["count"] * (luminance(r["radiance"]) if emissive else luminance(out_radiance))
        note("total_lum at 0", geometry & (total_lum != 0.0) & (np.abs(total_lum) < 1e-9))
        w = np.where(total_lum > 0.0, r["w_sum"] / total_lum, 0.0)
        out.render = np.where(geometry[..., None], np.concatenate([w[..., None] * out_radiance, np.ones((rh, rw, 1))], axis=-1), 0.0)
        out.minuend = r["w2_sum"] / r["count"]
        variance = out.minuend - (r["w_sum"] / r["count"]) ** 2
        divide = np.ones((rh, rw), bool) if mistake == "variance_always_divided" else ~(r["count"] < 1.0)
        variance = np.where(divide, variance / r["count"], variance)
        out.variance = np.where(np.isnan(variance), 10.0, np.minimum(variance, 10.0))
        out.variance_unit = np.where(divide, np.abs(out.minuend) / r["count"], np.abs(out.minuend))
    out.variance_written = geometry & use_variance
    out.stats = np.stack([np.where(geometry, r[k], cur[k]) for k in ("count", "w_sum", "w2_sum")], axis=-1)
    out.w = np.where(geometry, w, cur["w"])
    out.radiance_bits = np.where(geometry[..., None], r["radiance_bits"], cur["radiance_bits"])
    out.visible_position = np.where(geometry[..., None], r["visible_position"], cur["visible_position"]).astype(np.float32)
    out.lifetime = np.where(geometry, np.minimum(r["lifetime"] + 1.0, 254.0), cur["lifetime"])
    out.source, out.geometry, out.margin, out.open = source, geometry, margin & geometry, open_ & geometry
    out.reasons = {k: v & geometry for k, v in reasons.items()}
    return out


def f32_ulp(v):
    with np.errstate(all="ignore"):
        return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 23)


def check(e, planes, mistake=None):
    """one dispatch on the oracle against the restatement: ({quantity: worst deviation}, left-out share of the geometry pixels, the
    restatement, problems)"""
    PP.install_spatial(e, planes)
    e.pass_run(planes.pass_id)
    rw, rh = planes.render_size
    spatial = e.read(planes.outputs["spatial"]).reshape(-1, 16)[:rw * rh].reshape(rh, rw, 16)
    variance, render = e.read(planes.outputs["variance"])[..., 0], e.read(planes.outputs["render"])
    r = restate(planes, mistake)
    skip = r.margin | r.open
    problems, worst = [], {}
    halves = lambda word: np.stack([(spatial[..., word] & 0xFFFF).astype(np.uint16), (spatial[..., word] >> 16).astype(np.uint16)], axis=-1)
    got_stats = np.concatenate([halves(14), halves(15)], axis=-1)                       # count, w, w_sum, w2_sum
    want_stats = np.stack([r.stats[..., 0], r.w, r.stats[..., 1], r.stats[..., 2]], axis=-1)
    worst["render"], bad = deviation_f16(r.render, render, skip)
    if bad.any():
        problems.append(f"render: special values disagree at {int(bad.sum())} pixels, first {tuple(np.argwhere(bad)[0][::-1])}")
    worst["statistics"], bad = deviation_f16(want_stats, got_stats, skip)
    if bad.any():
        problems.append(f"statistics: special values disagree at {int(bad.sum())} pixels, first {tuple(np.argwhere(bad)[0][::-1])}")
    got_radiance = np.concatenate([halves(0), halves(1)], axis=-1)
    for label, differs in (("the radiance picked", (got_radiance != r.radiance_bits).any(axis=-1)),
                           ("the stored visible position", (spatial[..., 4:8] != r.visible_position.view(np.uint32)).any(axis=-1)),
                           ("the lifetime", ((spatial[..., 12] >> 24).astype(np.int64) != ((r.lifetime - 127.0).astype(np.int64) & 0xFF)))):
        differs = differs & ~skip
        if differs.any():
            problems.append(f"{label} disagrees at {int(differs.sum())} pixels, first {tuple(np.argwhere(differs)[0][::-1])}")
    written = r.variance_written
    stray = ~written & (variance != PP.SENTINEL_F32)
    if stray.any():
        problems.append(f"variance written at {int(stray.sum())} pixels that store none")
    with np.errstate(all="ignore"):
        capped = r.variance >= 10.0 - 1e-6
        dev = np.where(written & ~skip & ~capped & np.isfinite(r.variance), np.abs(variance.astype(np.float64) - r.variance) / f32_ulp(r.variance_unit), 0.0)
        wrong_cap = written & ~skip & (r.variance >= 10.0 + 1e-5) & (variance != np.float32(10.0))
    worst["variance"] = float(dev.max(initial=0.0))
    if wrong_cap.any():
        problems.append(f"variance above MAX_VARIANCE not clamped at {int(wrong_cap.sum())} pixels")
    n_geometry = int(r.geometry.sum())
    share = float(skip.sum()) / n_geometry if n_geometry else 0.0
    return worst, share, r, problems


# twice the worst deviation measured over every shape, ratio, parity and limit on `terraces`, rounded up to a whole ulp (DESIGN.md
# section 2): f16 ulps for `render` and the four statistics, f32 ulps of the minuend w2_sum / count for the variance.  The indirect
# channel's p goes through D_GGX, whose 1 - NoH * NoH cancels in f32 under the near-mirror materials of the scene (roughness 0.0079).
BOUNDS = {1: {"render": 33, "statistics": 1, "variance": 82}, 2: {"render": 30, "statistics": 21, "variance": 117784}}      # measured 16.229 0.500 40.83 | 14.762 10.476 58891.6
EXCLUDED_CAP = 0.02
SHAPES = [(w, h) for w in PP.SPATIAL_WIDTHS for h in PP.SPATIAL_HEIGHTS]
_measured = {}


def limits_of(k):
    return PP.SPATIAL_COUNTS[k % 3], PP.SPATIAL_LIFETIMES[(k // 3) % 3]


def settings():
    """every shape, ratio and parity; the nine (max count, lifetime limit) pairs rotate through them"""
    k = 0
    for shape in SHAPES:
        for ratio in PP.SPATIAL_RATIOS:
            for parity in (2, 3):
                yield shape, ratio, parity, limits_of(k)
                k += 1


def failures(planes, worst, share, r, problems):
    """what the comparison holds against one dispatch: discrete disagreements, a deviation above the channel's bound, more than 2 % of
    the geometry pixels left out (rounded up to a whole pixel under 585 pixels), a placed pixel of `terraces` left out"""
    bad = list(problems)
    bad += [f"{k}: {v:.3f} ulps, bound {BOUNDS[planes.channel][k]}" for k, v in worst.items() if v > BOUNDS[planes.channel][k]]
    n = int(r.geometry.sum())
    left_out = int((r.margin | r.open).sum())
    if left_out > (EXCLUDED_CAP * n if n >= 585 else np.ceil(EXCLUDED_CAP * n)):
        bad.append(f"{left_out} of {n} geometry pixels left out")
    if planes.name == "terraces" and (planes.placed & (r.margin | r.open)).any():
        bad.append(f"{int((planes.placed & (r.margin | r.open)).sum())} placed pixels left out")
    return bad


def branch_counts(r):
    c = {"merges": r.merges, "replaced": r.replaced, "kept": r.kept, "history_taken": r.history_taken, "history_refused": r.history_refused,
         "history_outside": r.history_outside, "clamped": r.clamped, "variance_written": r.variance_written, "variance_not_written": r.geometry & ~r.variance_written,
         "background": r.background}
    c.update({"reject_" + k: v for k, v in r.rejects.items()})
    c.update({f"march_end_{j}": v for j, v in r.march_end.items()})
    return {k: int(v.sum()) for k, v in c.items()}


@pytest.mark.parametrize("channel", [1, 2], ids=["emissive", "indirect"])
def test_oracle_agrees_with_float64_on_the_terraces(oracle, channel):
    bad, shares = {}, 0.0
    for shape, ratio, parity, (max_count, max_lifetime) in settings():
        planes = PP.make_spatial_planes("terraces", 7, shape, ratio, channel, parity, max_count, max_lifetime)
        worst, share, r, problems = check(oracle, planes)
        for k, v in worst.items():
            _measured[(channel, k)] = max(_measured.get((channel, k), 0.0), v)
        if shape[0] * shape[1] >= 585:
            shares = max(shares, share)
        b = failures(planes, worst, share, r, problems)
        if b:
            bad[(shape, ratio, parity, max_count, max_lifetime)] = b
    print("worst deviations", {k: round(v, 3) for k, v in _measured.items()}, "worst left-out share", round(shares, 4))
    assert bad == {}


ALL_BRANCHES = ["reject_" + k for k in REJECTS] + ["replaced", "kept", "history_taken", "history_refused", "clamped", "variance_written", "variance_not_written", "background"] + \
    [f"march_end_{j}" for j in range(1, 6)]
#: the branches each set is built for (the restatement's counts over the 70- and 49-wide shapes, every ratio, parity and limit, both channels)
WANT = {"terraces": ALL_BRANCHES, "random": ALL_BRANCHES + ["history_outside"],
        "depths": ["reject_outside", "reject_depth_ratio", "reject_occluded", "background", "merges"] + [f"march_end_{j}" for j in range(1, 6)],
        "records": ["reject_empty_or_normal", "reject_facing_away", "replaced", "kept", "clamped", "variance_written", "variance_not_written", "history_taken", "history_refused", "history_outside"],
        "history": ["history_taken", "history_refused", "history_outside"],
        "background": ["background", "merges", "reject_depth_ratio", "variance_written"]}


@pytest.mark.parametrize("name", PP.SPATIAL_SETS)
def test_every_set_runs_the_branches_it_was_built_for(name):
    total = {}
    for shape, ratio, parity, (max_count, max_lifetime) in settings():
        if shape[0] < 49:
            continue
        for channel in (1, 2):
            r = restate(PP.make_spatial_planes(name, 7, shape, ratio, channel, parity, max_count, max_lifetime))
            for k, v in branch_counts(r).items():
                total[k] = total.get(k, 0) + v
    print(name, total)
    assert [k for k in WANT[name] if total.get(k, 0) == 0] == []


def test_the_clamp_set_crosses_its_count_exactly_by_one_and_not_at_all():
    """`records`: a centre of half the maximum with no history whose taps are empty but one - the merged count is max, max + 1, max - 1"""
    for max_count in PP.SPATIAL_COUNTS:
        planes = PP.make_spatial_planes("records", 7, (70, 45), 1.0, 2, 2, max_count, 7.0)
        r = restate(planes)
        seen = {}
        for k, extra in enumerate((0, 1, -1)):
            x, y = 8 + 20 * k, 16
            assert not r.history_taken[y, x]
            seen[extra] = bool(r.clamped[y, x])
        assert seen[1] and not seen[0] and not seen[-1], (max_count, seen)


@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_comparison_notices_a_planted_mistake(oracle, mistake):
    """Negative control: the restatement with `>=` for `>` in the march, 0.9 for 0.866, the Jacobian dropped, the clamp dropped, the
    visible position not restored after the history load, eight taps for sixteen, the record tests not guarding the merge and the
    variance divided by a count below 1 must each fail the comparison - on the planes where the oracle passes it unplanted.  (`>=` for
    `>` shows on the `depths` set alone, at the occluder placed EXACTLY 1e-5 above the interpolated depth: the march comparison is
    replayed in f32, so a texel on that threshold is no margin.  The variance rule shows on `records`, which holds counts below 1, and
    so does 0.9: the normals of `terraces` are 15, 40 and 55 degrees apart by design, `records` places one at 28.)"""
    name = {"march_ge": "depths", "variance_always_divided": "records", "normal_09": "records"}.get(mistake, "terraces")
    caught = 0
    for ratio, parity, channel, max_count, max_lifetime in ((1.0, 2, 2, 100, 7.0), (1.5, 3, 2, 4, 0.0), (1.0, 3, 1, 100, 7.0)):
        planes = PP.make_spatial_planes(name, 7, (70, 45), ratio, channel, parity, max_count, max_lifetime)
        unplanted = failures(planes, *check(oracle, planes))
        if name != "records":      # (`records` holds what WGSL leaves open - NaN counts and weights under min, max and compares - and is not bounded: there the planted mistake must ADD disagreements)
            assert unplanted == []
        caught += failures(planes, *check(oracle, planes, mistake)) != unplanted
    assert caught, mistake


# ---------------------------------------------------------------- the shader's own word: tests/golden/wgsl_spatial_planes_*.npz
def shader_fixture_cases():
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import wgsl_pin

    return wgsl_pin


def replay_spatial_planes(e, case):
    """tests/golden/wgsl_spatial_planes_<case>.npz holds what the REFERENCE'S SHADER - spatial_reuse of light.wgsl, with and without
    EMISSIVE_LIT - wrote on the compact planes of `case` at 24 x 16: `spatial` (the records the pass indexes), `variance`, `render`
    (tests/tools/wgsl_pin.py --spatial-planes --write, run where the reference is at hand).  Run engine `e` on the same planes and
    return the buffers whose bytes differ from what the shader wrote."""
    wgsl_pin = shader_fixture_cases()
    name, channel, ratio, frame_number, max_count, max_lifetime = case
    data = np.load(wgsl_pin.spatial_planes_fixture_path(*case))
    planes = PP.make_spatial_planes(name, 7, (24, 16), ratio, channel, frame_number, max_count, max_lifetime, compact=True)
    PP.install_spatial(e, planes)
    e.pass_run(planes.pass_id)
    assert sorted(int(k.split("buf")[1]) for k in data.files) == sorted(planes.outputs.values())
    bad = []
    for key in data.files:
        got = e.read(int(key.split("buf")[1])).view(np.uint8).reshape(-1)
        differs = got[:data[key].size] != data[key]
        if differs.any():
            bad.append((key, int(differs.sum())))
    return bad


SPATIAL_PLANES_FIXTURES = shader_fixture_cases().SPATIAL_PLANES_FIXTURES
_ids = lambda c: f"{c[0]}-ch{c[1]}-r{int(c[2] * 10)}-f{c[3]}"


def test_the_fixtures_cover_what_they_are_for():
    cases = SPATIAL_PLANES_FIXTURES
    assert {c[0] for c in cases} == set(PP.SPATIAL_SETS) and {c[1] for c in cases} == {1, 2}
    assert {c[2] for c in cases} == {1.0, 1.5} and {c[3] % 2 for c in cases} == {0, 1}


@pytest.mark.parametrize("case", SPATIAL_PLANES_FIXTURES, ids=_ids)
def test_oracle_equals_what_the_reference_shader_wrote_on_the_planes(oracle, case):
    assert replay_spatial_planes(oracle, case) == []


@pytest.mark.skipif(not shader_fixture_cases().reference_available(), reason="no reference checkout (HIKARI_REFERENCE_DIR)")
@pytest.mark.parametrize("case", SPATIAL_PLANES_FIXTURES, ids=_ids)
def test_reference_shader_reproduces_the_oracle_on_the_planes(case):
    """spatial_reuse of light.wgsl itself, executed on the oracle's state: byte for byte, and the committed fixture is what it writes"""
    wgsl_pin = shader_fixture_cases()
    results = wgsl_pin.run_spatial_planes(*case)
    assert results and [r for r in results if r["mismatch"]] == []
    data = np.load(wgsl_pin.spatial_planes_fixture_path(*case))
    assert sorted(data.files) == sorted(wgsl_pin.run_spatial_planes.recorded)
    assert all((data[k] == wgsl_pin.run_spatial_planes.recorded[k]).all() for k in data.files)
