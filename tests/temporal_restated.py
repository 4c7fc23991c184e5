"""The three temporal light passes restated in float64 from the shader's text and bevy_pbr 0.9.1's lighting functions - direct_lit with
RENDER_EMISSIVE (the sun, channel 0) and with EMISSIVE_LIT (channel 1), light.wgsl:1040-1240; indirect_lit_ambient at one bounce (channel 2),
1262-1497; check_previous_reservoir / temporal_restir 917-952, update_reservoir / set_reservoir 138-170, select_light_candidate's
directional part 599-621, input_radiance 835-867 - for the planes of post_planes.make_temporal_planes on the OPEN scene, every pixel at once.

On the open scene every triangle lies below every surface point's tangent plane, so a ray that leaves the upper hemisphere of the
visible normal hits nothing and every new sample is analytic.  The sun: its colour where the cone direction has a positive cosine, the
sample at position + direction * 65535; a validation ray to a history sample finds the sun's colour inside the cone and nothing outside.
The emitters: the light tree is empty, no candidate, nothing traced - a black sample, w_new 0, and a validation that always replaces (its
ratio is 0).  Indirect: a cosine-weighted direction about the NORMALISED normal misses, the sample is the ambient colour with alpha 0 at
origin + direction * 65535, w_new = luminance(shading) / pdf; the output is shaded with the reservoir's own visible point before the
pixel's is put back.  A pixel whose validation ray leaves BELOW the surface, or whose colour is no number, is `open`.

Replayed in f32, where it is exact: the noise lookup and fract(. + number * golden), fract(dot(random, 1)), previous_uv and the index
arithmetic (post_planes.temporal_target), the validation frame's parity.  Every other decision is taken in float64 and noted in
`margin[reason]` where its operands lie within rounding of the threshold.  `branches` holds one boolean plane per outcome."""
import numpy as np

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F
from test_spatial_planes import F32, PI, dot, luminance, normalize, shading, unpack

MISTAKES = ("store_lt", "depth_100", "normal_0866", "count_le_4", "ratios_swapped", "no_clamp", "visible_not_restored", "lowest_wins")
REASONS = ("depth", "normal", "cosine", "cone", "pick", "luminance", "total")
_f32 = np.float32
TAU, GOLDEN, DISTANCE_MAX, RAY_BIAS, MAX_VARIANCE, EPS = F32(6.283185307), _f32(1.618033989), F32(65535.0), F32(0.02), F32(10.0), _f32(1.1920929e-7)


class Restated:
    pass


def normal_basis(n):
    """utils.wgsl:41-48: columns t, b, n"""
    s = np.minimum(np.sign(n[..., 2]) * 2.0 + 1.0, 1.0)
    u = -1.0 / (s + n[..., 2])
    v = n[..., 0] * n[..., 1] * u
    t = np.stack([1.0 + s * n[..., 0] * n[..., 0] * u, s * v, -s * n[..., 0]], axis=-1)
    b = np.stack([v, s + n[..., 1] * n[..., 1] * u, -n[..., 1]], axis=-1)
    return t, b


def cone_direction(sun, cos_angle, rand_zw):
    """normal_basis(cone.xyz) * sample_uniform_cone(rand.zw, cone.w).xyz (light.wgsl:552-559, 611-613)"""
    z = 1.0 - (1.0 - cos_angle) * rand_zw[..., 0]
    theta = TAU * rand_zw[..., 1]
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    t, b = normal_basis(np.broadcast_to(sun, rand_zw.shape[:-1] + (3,)))
    return t * (r * np.cos(theta))[..., None] + b * (r * np.sin(theta))[..., None] + sun * z[..., None]


def randoms(p):
    """s.random per render pixel in f32 (light.wgsl:1075-1079): [rh, rw, 4] float32"""
    rw, rh = p.render_size
    n = int(p.frame.number)
    noise = hk.load_noise().reshape(16, 64, 64, 4)[n % 16]
    ys, xs = (np.arange(rh) + n) % 64, (np.arange(rw) + n) % 64
    t = (noise[np.ix_(ys, xs)].astype(np.float32) / _f32(255.0)).astype(np.float32)
    s = (t + _f32(_f32(n) * GOLDEN)).astype(np.float32)
    return (s - np.floor(s)).astype(np.float32)


def fract_sum(random32):
    """fract(dot(random, vec4(1))) in f32, the products summed in order (light.wgsl:155)"""
    s = random32[..., 0]
    for k in (1, 2, 3):
        s = (s + random32[..., k]).astype(np.float32)
    return (s - np.floor(s)).astype(np.float32)


def restate(p, mistake=None):
    assert p.scene == "open" and mistake in (None,) + MISTAKES
    ch = p.channel
    (dw, dh), (rw, rh) = p.window_size, p.render_size
    fr, out = p.frame, Restated()
    position, velocity = p.buffers[F.BUF_POSITION], p.buffers[F.BUF_VELOCITY_UV]
    normal_bytes = p.buffers[F.BUF_NORMAL].view(np.int8).reshape(dh, dw, 4)
    ids = p.buffers[F.BUF_INSTANCE_MATERIAL]
    margin = {k: np.zeros((rh, rw), bool) for k in REASONS}
    # ---- per pixel, in f32: the G-buffer texel, previous_uv, the two conditions and the slot
    texel = np.zeros((rh, rw, 2), np.int64)
    inside = np.zeros((rh, rw), bool)
    loads, stores = np.zeros((rh, rw), bool), np.zeros((rh, rw), bool)
    slot = np.full((rh, rw), -1, np.int64)
    for y in range(rh):
        for x in range(rw):
            tx, ty = PP.spatial_texel(p, x, y)
            inside[y, x] = 0 <= tx < dw and 0 <= ty < dh
            texel[y, x] = (ty, tx) if inside[y, x] else (0, 0)
    ty, tx = texel[..., 0], texel[..., 1]
    depth = np.where(inside, position[ty, tx, 3], _f32(0.0))
    with np.errstate(all="ignore"):
        background = depth < EPS
    if ch == 2 and int(fr.indirect_bounces) == 0:
        background = np.ones((rh, rw), bool)
    geometry = ~background
    for y, x in zip(*np.nonzero(geometry)):
        (u, v), ld, st, index = PP.temporal_target(p, x, y, velocity[ty[y, x], tx[y, x], :2])
        if mistake == "store_lt":
            st = ld
        loads[y, x], stores[y, x] = ld, st
        if st:
            slot[y, x] = index
        if ld:                                                       # the load's own index (light.wgsl:181-190): the same arithmetic
            assert 0 <= index < rw * rh
    pos = position[ty, tx, :3].astype(np.float64)
    depth64 = depth.astype(np.float64)
    normal = np.maximum(normal_bytes[ty, tx, :3].astype(np.float64) / 127.0, -1.0)            # textureLoad of rgba8snorm: direct_lit does not normalise it
    open_ = np.zeros((rh, rw), bool)
    if ch == 2:                                                                                # indirect_lit_ambient does (light.wgsl:1288)
        normal = normalize(normal)
        open_ |= geometry & ~np.isfinite(normal).all(axis=-1)
    with np.errstate(all="ignore"):
        instance = np.trunc(np.nan_to_num(ids[ty, tx, 0].astype(np.float64), nan=0.0)).clip(0, 4294967295.0)
        material = np.trunc(np.nan_to_num(ids[ty, tx, 1].astype(np.float64), nan=0.0)).clip(0, len(PP.SPATIAL_MATERIALS) - 1).astype(np.int64)
    random32 = randoms(p)
    random = random32.astype(np.float64)

    # ---- history: the record under previous_uv, or a zero one; check_previous_reservoir (light.wgsl:917-935)
    h = unpack(p.previous)
    flat = np.where(loads, slot, 0)
    hy, hx = np.where(loads, flat // rw, 0), np.where(loads, flat % rw, 0)
    r = {k: np.where(loads.reshape(loads.shape + (1,) * (v.ndim - 2)), v[hy, hx], np.zeros_like(v[hy, hx])) for k, v in h.items()}
    with np.errstate(all="ignore"):                                  # (Sample.visible_instance is a u32: unpack converts the stored f32, a NaN to 0)
        stored_instance = np.trunc(np.nan_to_num(p.previous.visible_instance[hy, hx].astype(np.float64), nan=0.0)).clip(0, 4294967295.0)
    r["visible_instance"] = np.where(loads, stored_instance, 0.0)
    with np.errstate(all="ignore"):
        ratio = r["visible_position"][..., 3] / depth64
        ratio = np.where(ratio < 1.0, 1.0 / ratio, ratio)
        thr = F32(1.05 if mistake != "depth_100" else 1.0) * (1.0 + F32(0.5) * random[..., 0])
        depth_miss = ratio > thr
        margin["depth"] = geometry & (np.abs(ratio - thr) <= thr * 2.0 ** -21)
        instance_miss = r["visible_instance"] != instance
        cosine = dot(normal, r["visible_normal"])
        limit = F32(0.9) if mistake != "normal_0866" else F32(0.866)
        normal_miss = cosine < limit
        margin["normal"] = geometry & (np.abs(cosine - limit) <= 2.0 ** -20)
    passed = geometry & ~(depth_miss | normal_miss | instance_miss)
    br = {"background": background, "outside": geometry & ~stores, "history_taken": passed,
          "refused_depth_alone": geometry & loads & depth_miss & ~normal_miss & ~instance_miss,
          "refused_normal_alone": geometry & loads & normal_miss & ~depth_miss & ~instance_miss,
          "refused_instance_alone": geometry & loads & instance_miss & ~depth_miss & ~normal_miss,
          "refused": geometry & ~passed}
    zero = lambda v: np.zeros_like(v)
    R = {k: np.where(passed.reshape(passed.shape + (1,) * (v.ndim - 2)), v, zero(v)) for k, v in r.items()}
    R["lifetime"] = np.where(passed, r["lifetime"], 0.0)
    stored_first = geometry & ~passed & stores

    with np.errstate(all="ignore"):
        table = PP.SPATIAL_MATERIALS
        rough = lambda q: np.clip(F32(q), F32(0.089), 1.0) ** 2
        surface = {"base_color": np.array([[F32(c) for c in mt[0]] for mt in table])[material], "metallic": np.array([F32(mt[1]) for mt in table])[material],
                   "roughness": np.array([rough(mt[2]) for mt in table])[material], "reflectance": np.array([F32(0.3 + 0.1 * k) for k in range(len(table))])[material],
                   "occlusion": 1.0}
        camera = hk.cornell_camera(*p.window_size).view_uniform()
        V = normalize(np.array([F32(camera.world_position[i]) for i in range(3)]) - pos)
        ambient_color = np.array([F32(p.lights.ambient_color[i]) for i in range(3)])

    # ---- the new sample.  Sun (light.wgsl:1108-1153): through its cone, unoccluded.  Emitters: the light tree is empty, no candidate, the
    # sample is black and w_new 0.  Indirect (1404-1450, one bounce): a cosine-weighted direction that misses into the ambient term
    sun = normalize(np.array([F32(p.lights.direction_to_light[i]) for i in range(3)]))
    sun_raw = np.array([F32(p.lights.direction_to_light[i]) for i in range(3)])
    colour = np.array([F32(p.lights.directional_color[i]) for i in range(3)])
    cos_angle = np.cos(F32(fr.solar_angle))
    interval = int(fr.direct_validate_interval) if ch == 0 else int(fr.emissive_validate_interval)
    validation = ch != 2 and int(fr.number) % interval == 0
    low = (R["count"] <= 4.0) if mistake == "count_le_4" else (R["count"] < 4.0)
    sampled = geometry & (low if validation else np.ones((rh, rw), bool))
    with np.errstate(all="ignore"):
        if ch == 2:
            assert int(fr.indirect_bounces) <= 1
            radius, theta = np.sqrt(random[..., 0]), 2.0 * PI * random[..., 1]
            local = np.stack([radius * np.cos(theta), radius * np.sin(theta)], axis=-1)
            z = np.sqrt(1.0 - dot(local, local))
            pdf = 2.0 * F32(0.159154943) * z
            t, b = normal_basis(normal)
            direction = t * local[..., :1] + b * local[..., 1:] + normal * z[..., None]
            S = {"radiance": np.broadcast_to(np.append(ambient_color, 0.0), (rh, rw, 4)).copy(), "random": random, "random32": random32,
                 "sample_position": pos + normal * RAY_BIAS + direction * DISTANCE_MAX, "sample_normal": np.zeros((rh, rw, 3))}
            S["radiance_bits"] = PP.f16_bits(S["radiance"])
            first = shading(V, normal, normalize(S["sample_position"] - pos), surface, S["radiance"], ambient_color)
            w_new = np.where(pdf > 0.0, luminance(first) / pdf, 0.0)
            margin["cosine"] |= geometry & (z <= 2.0 ** -12)         # (a grazing ray: pdf near 0)
        else:
            direction = cone_direction(sun_raw, cos_angle, random[..., 2:])
            cosn = dot(direction, normal)
            if ch == 0:
                margin["cosine"] |= sampled & (np.abs(cosn) <= 2.0 ** -20)
            lit = (cosn > 0.0) & (ch == 0)
            S = {"radiance": np.where(lit[..., None], np.append(colour, 1.0), np.zeros(4)), "random": random, "random32": random32,
                 "sample_position": pos + direction * DISTANCE_MAX, "sample_normal": np.zeros((rh, rw, 3))}
            S["radiance_bits"] = PP.f16_bits(S["radiance"])
            w_new = luminance(S["radiance"])
        merged = {k: v.copy() for k, v in R.items()}
        merged["w_sum"] = R["w_sum"] + w_new
        merged["w2_sum"] = R["w2_sum"] + w_new * w_new
        merged["count"] = R["count"] + 1.0
        pick_at = w_new / merged["w_sum"]
        rand = fract_sum(random32).astype(np.float64)
        picked = rand < pick_at
        margin["pick"] = sampled & (np.abs(rand - pick_at) <= 2.0 ** -20)
        for k in ("radiance", "random", "random32", "sample_position", "sample_normal", "radiance_bits"):
            merged[k] = np.where(picked.reshape(picked.shape + (1,) * (merged[k].ndim - 2)), S[k], R[k])
        merged["flag"] = np.where(picked, 0.0, R["flag"])
        merged["visible_position"] = np.where(picked[..., None], np.concatenate([pos, depth64[..., None]], axis=-1), R["visible_position"])
        merged["visible_normal"] = np.where(picked[..., None], normal, R["visible_normal"])
        m = float(fr.max_temporal_reuse_count)
        over = merged["count"] > m
        if mistake != "no_clamp":
            merged["w_sum"] = np.where(over, merged["w_sum"] * (m / merged["count"]), merged["w_sum"])
            merged["w2_sum"] = np.where(over, merged["w2_sum"] * (m / merged["count"]), merged["w2_sum"])
            merged["count"] = np.where(over, m, merged["count"])
    for k in R:
        R[k] = np.where(sampled.reshape(sampled.shape + (1,) * (R[k].ndim - 2)), merged[k], R[k])
    br.update({"sample_merged": sampled, "sample_picked": sampled & picked, "clamp_hit": sampled & over})

    # ---- the validation frame (light.wgsl:1156-1214)
    stored_second = np.zeros((rh, rw), bool)
    out.second = None
    br.update({"validation_traced": np.zeros((rh, rw), bool), "validation_replaced": np.zeros((rh, rw), bool), "validation_kept": np.zeros((rh, rw), bool)})
    if validation:
        with np.errstate(all="ignore"):
            cand = cone_direction(sun_raw, cos_angle, R["random"][..., 2:])
            ray = normalize(R["sample_position"] - pos)
            traced = geometry & (dot(cand, R["visible_normal"]) > 0.0) & (ch == 0)      # (no emitter: the emissive pass traces nothing)
            if ch == 0:
                margin["cosine"] |= geometry & (np.abs(dot(cand, R["visible_normal"])) <= 2.0 ** -20)
            open_ |= traced & ~(dot(ray, normal) > 1e-3)             # (leaves below the surface, or normalize(0))
            in_cone = dot(ray, sun_raw) >= cos_angle
            margin["cone"] = traced & (np.abs(dot(ray, sun_raw) - cos_angle) <= 2.0 ** -20)
            validate = np.where((traced & in_cone)[..., None], np.append(colour, 1.0), np.zeros(4))
            old = R["count"] >= 4.0
            S2 = {k: v.copy() for k, v in S.items()}
            for k, v in (("random", R["random"]), ("random32", R["random32"]), ("sample_position", R["visible_position"][..., :3] + cand * DISTANCE_MAX),
                         ("sample_normal", np.zeros((rh, rw, 3))), ("radiance", validate), ("radiance_bits", PP.f16_bits(validate))):
                S2[k] = np.where(old.reshape(old.shape + (1,) * (v.ndim - 2)), v, S[k])
            lum_ratio = luminance(validate) / np.maximum(luminance(R["radiance"]), F32(0.0001))
            hi, lo = (F32(1.25), F32(0.8)) if mistake != "ratios_swapped" else (F32(0.8), F32(1.25))
            replaced = geometry & ((lum_ratio > hi) | (lum_ratio < lo))
            margin["luminance"] = geometry & ((np.abs(lum_ratio - F32(1.25)) <= 2.0 ** -20) | (np.abs(lum_ratio - F32(0.8)) <= 2.0 ** -20))
            stored_second = replaced & stores
            w2 = luminance(S2["radiance"])
            fresh = {"count": np.ones((rh, rw)), "lifetime": np.zeros((rh, rw)), "w_sum": w2, "w2_sum": w2 * w2, "flag": np.zeros((rh, rw))}
            for k in ("radiance", "random", "random32", "sample_position", "sample_normal", "radiance_bits"):
                fresh[k] = S2[k]
            out.second = {"radiance_bits": R["radiance_bits"].copy(), "visible_position": R["visible_position"].astype(np.float32), "count": R["count"].copy()}
            for k, v in fresh.items():
                R[k] = np.where(replaced.reshape(replaced.shape + (1,) * (v.ndim - 2)), v, R[k])
        br.update({"validation_traced": traced, "validation_replaced": replaced, "validation_kept": geometry & ~replaced})

    # ---- the stores to previous_spatial: where they go, which are dropped, who wins a slot
    wants = stored_first | stored_second
    discarded = wants & (slot >= rw * rh)
    br.update({"store_discarded": discarded, "store_to_own_slot": wants & (slot == np.arange(rw * rh).reshape(rh, rw)),
               "store_scattered": wants & ~discarded & (slot != np.arange(rw * rh).reshape(rh, rw))})
    winner = np.full(rw * rh, -1, np.int64)                        # highest pixel index that stores to a slot; a background pixel stores to its own
    order = np.arange(rw * rh) if mistake != "lowest_wins" else np.arange(rw * rh)[::-1]
    for i in order:
        y, x = divmod(int(i), rw)
        if background[y, x]:
            winner[i] = i
        elif wants[y, x] and not discarded[y, x]:
            winner[slot[y, x]] = i
    out.winner, out.slot, out.stored_second = winner.reshape(rh, rw), slot, stored_second

    # ---- the tail (light.wgsl:1216-1259)
    with np.errstate(all="ignore"):
        if ch == 2:        # (light.wgsl:1473-1481: shaded with the reservoir's own visible point, BEFORE the pixel's is put back)
            shaded = shading(V, R["visible_normal"], normalize(R["sample_position"] - R["visible_position"][..., :3]), surface, R["radiance"], ambient_color)
            total = R["count"] * luminance(shaded)
        else:
            total = R["count"] * luminance(R["radiance"])
        margin["total"] = geometry & (np.abs(total) <= 2.0 ** -40) & (total != 0.0)
        w = np.where(total > 0.0, R["w_sum"] / total, 0.0)
        lifetime = R["lifetime"] + 1.0
        minuend = R["w2_sum"] / R["count"]
        variance = minuend - (R["w_sum"] / R["count"]) ** 2
        variance = np.where(R["count"] < 1.0, variance, variance / R["count"])
        variance = np.where(np.isnan(variance), MAX_VARIANCE, np.minimum(variance, MAX_VARIANCE))
        N = normal if mistake != "visible_not_restored" else R["visible_normal"]
        P = pos if mistake != "visible_not_restored" else R["visible_position"][..., :3]
        L = normalize(R["sample_position"] - P)
        open_ |= geometry & ~np.isfinite(L).all(axis=-1)
        render = (shaded if ch == 2 else shading(V, N, L, surface, R["radiance"], ambient_color)) * w[..., None]
        open_ |= geometry & ~np.isfinite(render).all(axis=-1)
    out.geometry, out.background, out.open = geometry, background, open_ & geometry
    out.margin, out.reasons = np.logical_or.reduce([margin[k] for k in REASONS]) & geometry, margin
    out.branches = br
    out.count, out.w, out.w_sum, out.w2_sum, out.lifetime = R["count"], w, R["w_sum"], R["w2_sum"], lifetime
    out.radiance_bits, out.variance, out.variance_unit = R["radiance_bits"], variance, minuend
    out.visible_position = np.concatenate([position[ty, tx, :3], depth[..., None]], axis=-1).astype(np.float32) if mistake != "visible_not_restored" \
        else R["visible_position"].astype(np.float32)
    out.render = np.concatenate([render, np.ones((rh, rw, 1))], axis=-1)
    return out
