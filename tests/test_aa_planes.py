"""The oracle's anti-aliasing / upscale tail - taa.wgsl, smaa.wgsl (both entries), FsrEasuF and FsrRcasF - against a float64
restatement of the shaders on the adversarial planes of tests/post_planes.py (`make_aa_planes`), one dispatch at a time, in the
chain and with every pass alone on the written planes.

The restatement is written from the shaders' text and the FSR headers alone and uses none of the numeric contract's functions.  The
shader's order of operations decides every discrete choice; per pixel it returns the output, one mask per decision (boundary, depth,
position, velocity and instance miss, the clear colour, the clip branch, the corner offset and its ties, `zro`), a `margin` mask (its
own decision lies within rounding distance of a threshold: a nearest or footprint coordinate within 1e-4 of a texel boundary, a
bilinear weight of 0 against a non-finite texel, a reprojection so far outside that f32 holds no fraction of the sample position,
EASU's lobes cancelling) and a `dont_care` mask (what WGSL / GLSL leave open: min, max or clamp of a NaN, sqrt of a residue that
is zero but for rounding, the coordinate of a non-finite uv, floor / fract / cos of a non-finite).  FSR's approximate reciprocals
are restated bit-exactly on the f32 operand, everything else is carried in float64.

Outside both masks the oracle must agree in NaN-ness, the sign of an infinity and exact zeros and otherwise within BOUND_ULPS f16
ulps per kernel - twice the worst deviation measured over all sets, settings and shapes, rounded up.  For
TAA alone the unit is floored at 2^-20 of the texel's size (`deviation_floored`: it sums Catmull-Rom weights of either sign and clips
through a cancelling variance).  The shapes are those of RENDER_WIDTHS x RENDER_HEIGHTS.  At most 2 % of the texels a dispatch
writes may be left out, in the chain and alone, from 585 texels on (below: 2 % rounded up to a whole texel).  No texel a set placed -
its marks on all four grids, carried to each dispatch's grid through the uv - may be left out for a margin.  Two exemptions are
counted, not silent: the rows and columns of EASU and TAA whose own position is an input texel boundary EXACTLY (`line`: their
number follows from the two sizes), and for the placed-texel rule the pixels of SMAA Tu4x whose clip runs (`clip_margin`: its
gathers at previous_output_uv sit on G-buffer texel centres by construction at ratios 1 and 2).  The branches a set is for must
have run (WANT); planted mistakes must fail."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F
from test_post_chain_planes import deviation_f16, f16_ulp, half

# twice the measured worst deviations, rounded up to a whole ulp: DESIGN.md section 2
BOUND_ULPS = {"smaa_tu4x": 1, "smaa_tu4x_extrapolate": 2, "taa_jasmine": 11, "fsr_easu": 5, "fsr_rcas": 1}       # measured 0.499, 0.504, 5.006, 2.201, 0.500
EXCLUDED_CAP = 0.02
# the render shapes of RENDER_WIDTHS x RENDER_HEIGHTS with 585 texels and more
SHAPES = [(130, 17), (65, 17), (64, 17), (63, 17), (130, 9), (65, 9)]
EDGE_SHAPES = [(1, 1), (1, 9), (1, 17), (63, 1), (64, 1), (65, 1), (130, 1), (63, 9), (64, 9)]
LUMA = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], dtype=np.float64)
F32 = lambda v: float(np.float32(v))
TAU = F32(6.283185307)


class Open:
    """min / max / clamp / sqrt as numpy has them, remembering where WGSL and GLSL leave the result open"""

    def __init__(self, shape):
        self.mask = np.zeros(shape, bool)

    def _note(self, *operands):
        for a in operands:
            a = np.asarray(a)
            if a.ndim:
                self.mask |= np.isnan(a).reshape(a.shape[:2] + (-1,)).any(axis=2) if a.ndim > 2 else np.isnan(a)

    def min(self, a, b):
        self._note(a, b)
        return np.minimum(a, b)

    def max(self, a, b):
        self._note(a, b)
        return np.maximum(a, b)

    def clamp(self, a, lo, hi):
        self._note(a)
        return np.clip(a, lo, hi)


class Tex:
    """a plane in float64 with the two samplers of post_process.rs:679-690 (clamp-to-edge) and textureGather / textureLoad"""

    def __init__(self, data):
        self.d = np.asarray(data, dtype=np.float64)
        self.h, self.w = self.d.shape[:2]
        bad = self.bad = ~np.isfinite(self.d).all(axis=2)
        pad = np.pad(bad, 2)
        self.bad_near = np.zeros_like(bad)                      # a non-finite texel within two texels: a footprint one texel to either side reaches it
        for oy in range(5):
            for ox in range(5):
                self.bad_near |= pad[oy:oy + self.h, ox:ox + self.w]

    def _coords(self, u, v, shift):
        """floor(uv * size - shift) with clamp-to-edge in mind: the integer parts, the fractions, `close` (within 1e-4 of a boundary
        that changes the texels taken) and `open` (a non-finite coordinate)"""
        with np.errstate(all="ignore"):
            px, py = u * self.w - shift, v * self.h - shift
            open_ = ~(np.isfinite(px) & np.isfinite(py))
            px, py = np.where(open_, 0.0, px), np.where(open_, 0.0, py)
            lo = 0.5 - shift                                    # nearest: boundaries 1 .. size - 1; footprint: 0 .. size - 1
            close = ((np.abs(px - np.rint(px)) < 1e-4) & (px > lo - 0.5) & (px < self.w - 0.5)) | ((np.abs(py - np.rint(py)) < 1e-4) & (py > lo - 0.5) & (py < self.h - 0.5))
            fx, fy = np.floor(px), np.floor(py)
        return fx, fy, px - fx, py - fy, close & ~open_, open_

    def _ix(self, f, n):
        return np.clip(f, 0, n - 1).astype(np.int64)

    def nearest(self, u, v):
        fx, fy, _, _, close, open_ = self._coords(u, v, 0.0)
        return self.d[self._ix(fy, self.h), self._ix(fx, self.w)], close, open_

    def gather(self, component, u, v):
        """x = (u_min, v_max), y = (u_max, v_max), z = (u_max, v_min), w = (u_min, v_min)"""
        fx, fy, _, _, close, open_ = self._coords(u, v, 0.5)
        x0, x1, y0, y1 = self._ix(fx, self.w), self._ix(fx + 1, self.w), self._ix(fy, self.h), self._ix(fy + 1, self.h)
        c = self.d[..., component]
        order = [(y1, x0), (y1, x1), (y0, x1), (y0, x0)]
        return np.stack([c[yy, xx] for yy, xx in order], axis=-1), close, open_

    def linear(self, u, v):
        fx, fy, tx, ty, close, open_ = self._coords(u, v, 0.5)
        x0, x1, y0, y1 = self._ix(fx, self.w), self._ix(fx + 1, self.w), self._ix(fy, self.h), self._ix(fy + 1, self.h)
        tx, ty = tx[..., None], ty[..., None]
        with np.errstate(all="ignore"):
            top = self.d[y0, x0] * (1.0 - tx) + self.d[y0, x1] * tx
            bottom = self.d[y1, x0] * (1.0 - tx) + self.d[y1, x1] * tx
            out = top * (1.0 - ty) + bottom * ty
        # A weight of exactly 0 against a non-finite texel: 0 * Inf is NaN, 1e-9 * Inf is not, and at a fraction within 1e-4 of 0 or
        # 1 f32 may have taken the footprint one texel over.  The hazard is a non-finite texel in the row (column) that has, or would
        # then have, the weight 0 - beside the footprint on either side, or its far half.
        bad = lambda fy_, fx_: self.bad[self._ix(fy_, self.h), self._ix(fx_, self.w)]
        cols = lambda fy_: bad(fy_, fx - 1) | bad(fy_, fx) | bad(fy_, fx + 1) | bad(fy_, fx + 2)
        rows = lambda fx_: bad(fy - 1, fx_) | bad(fy, fx_) | bad(fy + 1, fx_) | bad(fy + 2, fx_)
        tx, ty = tx[..., 0], ty[..., 0]
        hazard = ((ty < 1e-4) & (cols(fy - 1) | cols(fy + 1))) | ((ty > 1 - 1e-4) & (cols(fy) | cols(fy + 2)))
        hazard |= ((tx < 1e-4) & (rows(fx - 1) | rows(fx + 1))) | ((tx > 1 - 1e-4) & (rows(fx) | rows(fx + 2)))
        return out, hazard & ~open_, open_

    def load(self, x, y):
        inside = (x >= 0) & (y >= 0) & (x < self.w) & (y < self.h)
        return np.where(inside[..., None], self.d[np.clip(y, 0, self.h - 1), np.clip(x, 0, self.w - 1)], 0.0)


def rgb_to_ycocg(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([(r / 4.0) + (g / 2.0) + (b / 4.0), (r / 2.0) - (b / 2.0), (-r / 4.0) + (g / 2.0) - (b / 4.0)], axis=-1)


def ycocg_to_rgb(o, y):
    return o.clamp(np.stack([y[..., 0] + y[..., 1] - y[..., 2], y[..., 0] + y[..., 2], y[..., 0] - y[..., 1] - y[..., 2]], axis=-1), 0.0, 1.0)


def clip_towards_aabb_center(o, previous, aabb_min, aabb_max):
    p_clip = 0.5 * (aabb_max + aabb_min)
    e_clip = 0.5 * (aabb_max - aabb_min)
    v_clip = previous - p_clip
    a_unit = np.abs(v_clip / e_clip)
    ma_unit = o.max(a_unit[..., 0], o.max(a_unit[..., 1], a_unit[..., 2]))
    clipped = ma_unit > 1.0
    unit = v_clip / e_clip
    KINDS.update(pos_inf=(unit == np.inf).any(axis=-1), neg_inf=(unit == -np.inf).any(axis=-1), zero_over_zero=((v_clip == 0.0) & (e_clip == 0.0)).any(axis=-1))
    return np.where(clipped[..., None], p_clip + v_clip / ma_unit[..., None], previous), clipped


KINDS = {}          # what the last clip_towards_aabb_center / variance_box met, per pixel: +Inf, -Inf and 0 / 0 in `v_clip / e_clip`, a flat residue


def variance_box(o, samples):
    """mean -+ sqrt(moment_2 / n - mean^2) of the samples; where the residue is zero but for rounding the sqrt is of a number f32 may
    have made negative: open"""
    n = float(len(samples))
    moment_1, moment_2 = sum(samples[1:], samples[0]), sum((s * s for s in samples[1:]), samples[0] * samples[0])
    mean = moment_1 / n
    residue = moment_2 / n - mean * mean
    o.mask |= (residue <= 1e-6 * np.abs(moment_2 / n)).any(axis=-1) | np.isnan(residue).any(axis=-1)
    KINDS["flat_residue"] = (np.abs(residue) <= 1e-6 * np.abs(moment_2 / n)).all(axis=-1) & (moment_2 > 0.0).any(axis=-1)
    variance = np.sqrt(np.maximum(residue, 0.0))
    return mean - variance, mean + variance


def nearest_velocity(o, margin, position, velocity, u, v, tx, ty, mistake=None):
    """taa.wgsl:54-73 / smaa.wgsl:52-71; returns the velocity and whether the offset was taken"""
    corners = [(tx, ty), (-tx, ty), (tx, -ty), (-tx, -ty)]
    depths = []
    for ox, oy in corners:
        t, close, open_ = position.nearest(u + ox, v + oy)
        margin |= close
        o.mask |= open_
        depths.append(t[..., 3])
    max_depth = o.max(o.max(depths[0], depths[1]), o.max(depths[2], depths[3]))
    t, close, open_ = position.nearest(u, v)
    margin |= close
    o.mask |= open_
    moved = t[..., 3] < max_depth
    signs_x, signs_y = (1.0, -1.0, 1.0, -1.0), ((1.0, 1.0, -1.0, -1.0) if mistake != "swapped_corners" else (-1.0, -1.0, 1.0, 1.0))
    ox = sum(np.where(d == max_depth, s * tx, 0.0) for d, s in zip(depths, signs_x))
    oy = sum(np.where(d == max_depth, s * ty, 0.0) for d, s in zip(depths, signs_y))
    vel, close, open_ = velocity.nearest(u + np.where(moved, ox, 0.0), v + np.where(moved, oy, 0.0))
    margin |= close
    o.mask |= open_
    ties = sum((d == max_depth).astype(int) for d in depths)
    return vel[..., :2], moved, ties


def length(a):
    return np.sqrt((a * a).sum(axis=-1))


def ref_taa(render, previous_render, position, velocity, previous_position, previous_velocity, size, ratio, clear, mistake=None):
    tw, th = size
    render, previous_render, position, velocity = Tex(half(render)), Tex(half(previous_render)), Tex(position), Tex(velocity)
    previous_position, previous_velocity = Tex(previous_position), Tex(previous_velocity)
    y, x = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
    o, margin = Open((th, tw)), np.zeros((th, tw), bool)
    with np.errstate(all="ignore"):
        tsx, tsy = 1.0 / tw, 1.0 / th
        u, v = (x + 0.5) / tw, (y + 0.5) / th
        original, close, _ = render.nearest(u, v)
        margin |= close
        current = original[..., :3]
        vel, moved, ties = nearest_velocity(o, margin, position, velocity, u, v, 1.0 / render.w, 1.0 / render.h, mistake)
        pu, pv = u - vel[..., 0], v - vel[..., 1]
        boundary = (np.abs(pu - 0.5) > 0.5) | (np.abs(pv - 0.5) > 0.5)
        margin |= (np.abs(np.abs(pu - 0.5) - 0.5) < 1e-6) | (np.abs(np.abs(pv - 0.5) - 0.5) < 1e-6)
        cpd, close, _ = position.nearest(u, v)
        cd = cpd[..., 3]
        has_content, depth_miss, position_miss = cd > 0.0, cd == 0.0, cd == 0.0
        positive, slots = np.zeros((th, tw), int), []
        for bx, by in [(0.0, 0.0), (1.5, 1.5), (-1.5, 1.5), (1.5, -1.5), (-1.5, -1.5)]:
            su, sv = pu + bx * tsx, pv + by * tsy
            pd, close, open_ = previous_position.gather(3, su, sv)
            margin |= close
            o.mask |= open_
            ratio_ = np.where(pd == 0.0, 1.0, cd[..., None] / pd)
            has_content = has_content | (pd > 0.0).any(axis=-1)
            positive += (pd > 0.0).sum(axis=-1)
            slots.append(pd > 0.0)
            depth_miss = depth_miss | (ratio_ < F32(0.95)).any(axis=-1)
            margin |= (np.abs(ratio_ - F32(0.95)) < 1e-6).any(axis=-1)
            pp, close, open_ = previous_position.nearest(su, sv)
            margin |= close
            o.mask |= open_
            distance = length(cpd[..., :3] - pp[..., :3])
            position_miss = position_miss | (distance > 0.5)
            margin |= np.abs(distance - 0.5) < 1e-6
        pvel, close, open_ = previous_velocity.nearest(pu, pv)
        margin |= close
        o.mask |= open_
        dv = length(vel - pvel[..., :2])
        velocity_miss = dv > F32(0.00005)
        margin |= np.abs(dv - F32(0.00005)) < 4e-7 * np.maximum(np.abs(vel).max(axis=-1), np.abs(pvel[..., :2]).max(axis=-1)) + 1e-10
        # 5-tap Catmull-Rom
        spx, spy = pu * tw, pv * th
        o.mask |= ~(np.isfinite(spx) & np.isfinite(spy))                   # floor of a non-finite
        margin |= (np.abs(spx) > 2.0 ** 16) | (np.abs(spy) > 2.0 ** 16)     # (f32 holds no usable fraction of the sample position out there)
        spx, spy = np.where(np.isfinite(spx), spx, 0.0), np.where(np.isfinite(spy), spy, 0.0)
        t1x, t1y = np.floor(spx - 0.5) + 0.5, np.floor(spy - 0.5) + 0.5
        previous = np.zeros((th, tw, 3))
        weights = []
        for f in (spx - t1x, spy - t1y):
            w0 = f * (-0.5 + f * (1.0 - 0.5 * f))
            w1 = 1.0 + f * f * (-2.5 + 1.5 * f)
            w2 = f * (0.5 + f * (2.0 - 1.5 * f))
            w3 = f * f * (-0.5 + 0.5 * f)
            weights.append((w3, w1 + w2, w0, w2 / (w1 + w2)) if mistake == "weights_swapped" else (w0, w1 + w2, w3, w2 / (w1 + w2)))
        (w0x, w12x, w3x, o12x), (w0y, w12y, w3y, o12y) = weights
        p0x, p3x, p12x = (t1x - 1.0) * tsx, (t1x + 2.0) * tsx, (t1x + o12x) * tsx
        p0y, p3y, p12y = (t1y - 1.0) * tsy, (t1y + 2.0) * tsy, (t1y + o12y) * tsy
        near_boundary = (np.abs((spx - 0.5) - np.rint(spx - 0.5)) < 1e-4) | (np.abs((spy - 0.5) - np.rint(spy - 0.5)) < 1e-4)
        for su, sv, wa, wb in [(p12x, p0y, w12x, w0y), (p0x, p12y, w0x, w12y), (p12x, p12y, w12x, w12y), (p3x, p12y, w3x, w12y), (p12x, p3y, w12x, w3y)]:
            c, close, open_ = previous_render.linear(su, sv)
            margin |= close
            previous = previous + o.clamp(c[..., :3], 0.0, 1.0) * wa[..., None] * wb[..., None]
        clip = boundary | (position_miss & velocity_miss & depth_miss)
        samples = []
        for offset in [(-tsx, tsy), (0.0, tsy), (tsx, tsy), (-tsx, 0.0), None, (tsx, 0.0), (-tsx, -tsy), (0.0, -tsy), (tsx, -tsy)]:
            if offset is None:
                samples.append(rgb_to_ycocg(current))
                continue
            c, close, _ = render.nearest(u + offset[0], v + offset[1])
            margin |= close & clip
            oc = Open((th, tw))
            samples.append(rgb_to_ycocg(oc.clamp(c[..., :3], 0.0, 1.0)))
            o.mask |= oc.mask & clip
        oc = Open((th, tw))
        lo, hi = variance_box(oc, samples)
        clipped, took = clip_towards_aabb_center(oc, rgb_to_ycocg(previous), lo, hi)
        clipped = ycocg_to_rgb(oc, clipped)
        o.mask |= oc.mask & clip
        previous = np.where(clip[..., None], clipped, previous)
        blend = F32(0.1) / F32(ratio)
        out = previous * (1.0 - blend) + current * blend
        o.mask |= (np.isinf(previous) & np.isinf(current)).any(axis=-1)       # (mix is x * (1 - a) + y * a or x + (y - x) * a)
        color = np.concatenate([out, original[..., 3:4]], axis=2)
        color = np.where(has_content[..., None], color, clear)
        empty = ~has_content
    masks = {"boundary": boundary & ~empty, "depth": depth_miss & ~empty, "position": position_miss & ~empty, "velocity": velocity_miss & ~empty,
             "clear": empty, "clip": clip & ~empty, "clip_taken": clip & took & ~empty, "offset": moved, "lone_depth": (positive == 1) & (cd == 0.0)}
    counts = {k: int(m.sum()) for k, m in masks.items()}
    counts.update({f"ties{k}": int(((ties == k) & moved).sum()) for k in (2, 3, 4)})
    counts.update({"clip_" + k: int((m & clip & ~empty).sum()) for k, m in KINDS.items()})
    lone = masks["lone_depth"]
    counts["lone_slots"] = sum(int((s[..., k] & lone).any()) for s in slots for k in range(4))       # of the 5 biases x 4 gather corners: how many saw the lone depth
    # the columns / rows whose own uv (or its neighbour one input texel over, nearest_velocity's corners) falls on a G-buffer texel
    # boundary EXACTLY - the middle column of a 63-wide image under a 94-wide G-buffer: left out, their number follows from the sizes
    with np.errstate(all="ignore"):
        line = np.zeros((th, tw), bool)
        for c, n, step in ((u, position.w, 1.0 / render.w), (v, position.h, 1.0 / render.h)):
            for s in (0.0, step, -step):
                q = (c + s) * n
                line |= (np.abs(q - np.rint(q)) < 1e-9) & (q > 0.5) & (q < n - 0.5)
    return {"out": color, "margin": margin & ~empty, "dont_care": o.mask & ~empty, "counts": counts, "masks": masks, "line": line & margin & ~empty}


def ref_smaa(render, previous_render, position, velocity, previous_position, previous_velocity, instance, out_size, frame_number, mistake=None):
    """smaa_tu4x: returns the two texels every thread stores, as planes on the render grid, and where they go"""
    ow, oh = out_size
    render, previous_render, position, velocity = Tex(half(render)), Tex(half(previous_render)), Tex(position), Tex(velocity)
    previous_position, previous_velocity, instance = Tex(previous_position), Tex(previous_velocity), Tex(instance)
    rw, rh = render.w, render.h
    y, x = np.meshgrid(np.arange(rh), np.arange(rw), indexing="ij")
    o, margin = Open((rh, rw)), np.zeros((rh, rw), bool)
    cj, pj = (0, 1) if (frame_number % 2 == 0) != (mistake == "jitter_swapped") else (1, 0)
    with np.errstate(all="ignore"):
        tsx, tsy = 1.0 / ow, 1.0 / oh
        current, close, _ = render.nearest((x + 0.5) / rw, (y + 0.5) / rh)
        current = current[..., :3]
        pox, poy = 2 * x + pj, 2 * y + pj
        u, v = (pox + 0.5) / ow, (poy + 0.5) / oh
        vel, moved, ties = nearest_velocity(o, margin, position, velocity, u, v, 1.0 / position.w, 1.0 / position.h, mistake)
        pu, pv = u - vel[..., 0], v - vel[..., 1]
        previous, close, open_ = previous_render.nearest(pu, pv)
        margin |= close
        o.mask |= open_
        previous = previous[..., :3]
        boundary = (np.abs(pu - 0.5) > 0.5) | (np.abs(pv - 0.5) > 0.5)
        margin |= (np.abs(np.abs(pu - 0.5) - 0.5) < 1e-6) | (np.abs(np.abs(pv - 0.5) - 0.5) < 1e-6)
        ci, close, _ = instance.nearest(u, v)
        margin |= close
        cdt, _, _ = position.nearest(u, v)
        cd = cdt[..., 3]
        depth_miss, instance_miss = cd == 0.0, np.zeros((rh, rw), bool)
        step_exact, step_ulp = np.zeros((rh, rw), bool), np.zeros((rh, rw), bool)
        biases = [(0.0, 0.0), (2.5, 2.5), (-2.5, 2.5), (2.5, -2.5), (-2.5, -2.5)]
        for bx, by in biases:
            su, sv = pu + bx * tsx, pv + by * tsy
            pd, close, open_ = previous_position.gather(3, su, sv)
            margin |= close
            o.mask |= open_
            ratio_ = np.where(pd == 0.0, 1.0, cd[..., None] / pd)
            any_ratio = (ratio_ < F32(0.95)).any(axis=-1)
            margin |= (np.abs(ratio_ - F32(0.95)) < 1e-6).any(axis=-1)
            depth_miss = depth_miss | any_ratio
            pi, close, open_ = instance.nearest(su, sv)
            margin |= close
            o.mask |= open_
            di = np.abs(pi[..., 0] - ci[..., 0])
            instance_miss = instance_miss | (any_ratio & (di > 1.0))
            step_exact, step_ulp = step_exact | (any_ratio & (di == 1.0)), step_ulp | (any_ratio & (di > 1.0) & (di < 1.0 + 1e-6))
            margin |= any_ratio & (np.abs(di - 1.0) < 1e-9) & (di != 1.0)
        pvel, close, open_ = previous_velocity.nearest(pu, pv)
        margin |= close
        o.mask |= open_
        dv = length(vel - pvel[..., :2])
        velocity_miss = dv > F32(0.0001)
        margin |= np.abs(dv - F32(0.0001)) < 4e-7 * np.maximum(np.abs(vel).max(axis=-1), np.abs(pvel[..., :2]).max(axis=-1)) + 1e-10
        clip = boundary | ((depth_miss | instance_miss) & velocity_miss)
        oc = Open((rh, rw))
        bias_x, bias_y, min_ds = np.zeros((rh, rw)), np.zeros((rh, rw)), np.full((rh, rw), 10.0)
        tie_margin = np.zeros((rh, rw), bool)
        for bx, by in biases:
            ds, close, _ = position.gather(3, u + bx * tsx, v + by * tsy)
            tie_margin |= close
            dds = length(cd[..., None] - ds)
            take = dds < min_ds
            tie_margin |= (np.abs(dds - min_ds) < 1e-6 * np.maximum(np.abs(cd), 1e-3)) & (dds != min_ds)
            bias_x, bias_y = np.where(take, bx * tsx, bias_x), np.where(take, by * tsy, bias_y)
            min_ds = oc.min(min_ds, dds)
        gathers = [render.gather(c, u + bias_x, v + bias_y) for c in range(3)]
        tie_margin |= gathers[0][1]
        samples = [rgb_to_ycocg(np.stack([gathers[c][0][..., k] for c in range(3)], axis=-1)) for k in range(4)]
        lo, hi = variance_box(oc, samples)
        clipped, took = clip_towards_aabb_center(oc, rgb_to_ycocg(previous), lo, hi)
        clipped = ycocg_to_rgb(oc, clipped)
        o.mask |= oc.mask & clip
        margin |= tie_margin & clip
        previous = np.where(clip[..., None], clipped, previous)
        svx, svy = vel[..., 0] / (2.0 * tsx), vel[..., 1] / (2.0 * tsy)
        o.mask |= ~(np.isfinite(svx) & np.isfinite(svy))                  # fract / cos of a non-finite
        margin |= (np.abs(svx) > 2.0 ** 12) | (np.abs(svy) > 2.0 ** 12)    # (f32 keeps too little of the fraction: cos moves by more than an ulp of the result)
        svx, svy = np.where(np.isfinite(svx), svx, 0.0), np.where(np.isfinite(svy), svy, 0.0)
        fx, fy = svx - np.floor(svx), svy - np.floor(svy)
        margin |= ((np.abs(svx - np.rint(svx)) < 1e-5) & (svx != np.rint(svx))) | ((np.abs(svy - np.rint(svy)) < 1e-5) & (svy != np.rint(svy)))    # fract jumps
        blend = o.clamp(-np.cos(o.max(fx, fy) * TAU), 0.0, 1.0)
        remix, close, _ = render.linear(u, v)
        margin |= close
        previous = previous * (1.0 - blend[..., None]) + remix[..., :3] * blend[..., None]
        o.mask |= (np.isinf(previous) & np.isinf(remix[..., :3])).any(axis=-1) | (~np.isfinite(remix[..., :3]).all(axis=-1) & (blend == 0.0)) | (~np.isfinite(previous).all(axis=-1) & (blend == 1.0))
        one = np.ones((rh, rw, 1))
    masks = {"boundary": boundary, "depth": depth_miss, "instance": instance_miss, "velocity": velocity_miss, "clip": clip, "clip_taken": clip & took, "offset": moved,
             "step_1_no_miss": step_exact & ~instance_miss, "step_1_ulp_miss": step_ulp}       # an id step of exactly 1.0 is no miss, one of 1 + ulp is
    counts = {k: int(m.sum()) for k, m in masks.items()}
    counts.update({"clip_" + k: int((m & clip).sum()) for k, m in KINDS.items()})
    counts.update({f"ties{k}": int(((ties == k) & moved).sum()) for k in (2, 3, 4)})
    return {"current": np.concatenate([current, one], axis=2), "previous": np.concatenate([previous, one], axis=2), "at": ((2 * x + cj, 2 * y + cj), (pox, poy)),
            "margin": margin, "dont_care": o.mask, "counts": counts, "masks": masks, "clip_margin": tie_margin & clip}


def ref_extrapolate(output_bits, render_size, mistake=None):
    """smaa_tu4x_extrapolate, in place: the two texels every thread stores, on the render grid"""
    t = Tex(half(output_bits))
    rw, rh = render_size
    y, x = np.meshgrid(np.arange(rh), np.arange(rw), indexing="ij")
    o = Open((rh, rw))
    lum = lambda c: np.abs(c[..., :3]) @ LUMA
    with np.errstate(all="ignore"):
        tc, bc, nc = t.load(2 * x, 2 * y), t.load(2 * x + 1, 2 * y + 1), t.load(2 * x + 1, 2 * y - 1)
        ec, sc, wc = t.load(2 * x + 2, 2 * y), t.load(2 * x, 2 * y + 2), t.load(2 * x - 1, 2 * y + 1)
        dh = (lum(wc - bc), lum(tc - ec))
        dv = (lum(tc - sc), lum(nc - bc))
        fx = o.max(dv[0], F32(0.001)) * o.max(dv[1], F32(0.001))
        fy = o.max(dh[0], F32(0.001)) * o.max(dh[1], F32(0.001))
        fz = 1.0 / (fx + fy)
        blend = lambda tt, bb, ll, rr: (0.5 * fz)[..., None] * ((ll + rr) * fx[..., None] + (tt + bb) * fy[..., None])
        xc, yc = (blend(wc, bc, tc, sc) if mistake == "transposed_blend" else blend(tc, sc, wc, bc)), blend(nc, bc, tc, ec)
        nonfinite = sum((~np.isfinite(c).all(axis=-1)).astype(int) for c in (tc, bc, nc, ec, sc, wc))
    return {"x": xc, "y": yc, "at": ((2 * x, 2 * y + 1), (2 * x + 1, 2 * y)), "margin": np.zeros((rh, rw), bool), "dont_care": o.mask,
            "counts": {"all_six_nonfinite": int((nonfinite == 6).sum()), "loads_touched": int((nonfinite > 0).sum()),
                       "floor_0001": int(((dv[0] < 0.001) | (dh[0] < 0.001)).sum())}}


def bits_f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.int64)


def from_bits(b):
    return (np.asarray(b, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64)


def prx_lo_rcp(a):          # ffx_a.h APrxLoRcpF1: on the f32 operand's bits
    return from_bits(0x7EF07EBB - bits_f32(a))


def prx_med_rcp(a):         # APrxMedRcpF1: one Newton step on the bit trick
    b = from_bits(0x7EF19FFF - bits_f32(a))
    return b * (-b * a + 2.0)


def prx_lo_rsq(a):          # APrxLoRsqF1
    return from_bits(0x5F347D74 - (bits_f32(a) >> 1))


def ref_easu(input_bits, out_size, mistake=None):
    t = Tex(half(input_bits))
    iw, ih = t.w, t.h
    ow, oh = out_size
    y, x = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    o = Open((oh, ow))
    with np.errstate(all="ignore"):
        # FsrEasuCon with the input viewport = the input size
        ppx, ppy = x * (iw / ow) + (0.5 * iw / ow - 0.5), y * (ih / oh) + (0.5 * ih / oh - 0.5)
        # (floor: at 1 : 1 the position is the pixel's own index in f32 as well; at any other ratio an integer is reached by rounding)
        margin = ((np.abs(ppx - np.rint(ppx)) < 1e-4) & (iw != ow)) | ((np.abs(ppy - np.rint(ppy)) < 1e-4) & (ih != oh))
        # ... and where it is an integer EXACTLY - the output pixel sits on an input texel boundary, as the middle row and column of an
        # image do whenever both sizes are odd, or even with odd halves - the line is left out whatever the planes hold: its length
        # follows from the two sizes, not from a share of the image, and it is not counted against the 2 %
        line = ((np.abs(ppx - np.rint(ppx)) < 1e-9) & (iw != ow)) | ((np.abs(ppy - np.rint(ppy)) < 1e-9) & (ih != oh))
        fpx, fpy = np.floor(ppx), np.floor(ppy)
        ppx, ppy = ppx - fpx, ppy - fpy
        fpx, fpy = fpx.astype(np.int64), fpy.astype(np.int64)
        tap = lambda dx, dy: t.d[np.clip(fpy + dy, 0, ih - 1), np.clip(fpx + dx, 0, iw - 1)][..., :3]       # fakeTextureGather: the texels around a corner, clamp-to-edge
        names = {"b": (0, -1), "c": (1, -1), "e": (-1, 0), "f": (0, 0), "g": (1, 0), "h": (2, 0), "i": (-1, 1), "j": (0, 1), "k": (1, 1), "l": (2, 1), "n": (0, 2), "o": (1, 2)}
        if mistake == "mirrored_taps":
            names = {k: (dx, 1 - dy) for k, (dx, dy) in names.items()}
        c = {k: tap(*d) for k, d in names.items()}
        L = {k: v[..., 2] * 0.5 + (v[..., 0] * 0.5 + v[..., 1]) for k, v in c.items()}
        dirx, diry, ln = np.zeros((oh, ow)), np.zeros((oh, ow)), np.zeros((oh, ow))

        def set_(w, lA, lB, lC, lD, lE):
            nonlocal dirx, diry, ln
            dc, cb = lD - lC, lC - lB
            lenx = prx_lo_rcp(o.max(np.abs(dc), np.abs(cb)))
            dx = lD - lB
            dirx = dirx + dx * w
            lenx = o.clamp(np.abs(dx) * lenx, 0.0, 1.0)
            ln = ln + lenx * lenx * w
            ec, ca = lE - lC, lC - lA
            leny = prx_lo_rcp(o.max(np.abs(ec), np.abs(ca)))
            dy = lE - lA
            diry = diry + dy * w
            leny = o.clamp(np.abs(dy) * leny, 0.0, 1.0)
            ln = ln + leny * leny * w

        set_((1.0 - ppx) * (1.0 - ppy), L["b"], L["e"], L["f"], L["g"], L["j"])
        set_(ppx * (1.0 - ppy), L["c"], L["f"], L["g"], L["h"], L["k"])
        set_((1.0 - ppx) * ppy, L["f"], L["i"], L["j"], L["k"], L["n"])
        set_(ppx * ppy, L["g"], L["j"], L["k"], L["l"], L["o"])
        dirr = dirx * dirx + diry * diry
        zro = dirr < 1.0 / 32768.0
        margin |= (np.abs(dirr - 1.0 / 32768.0) < 1e-9)
        rsq = np.where(zro, 1.0, prx_lo_rsq(dirr))
        dirx = np.where(zro, 1.0, dirx) * rsq
        diry = diry * rsq
        ln = ln * 0.5
        ln = ln * ln
        stretch = (dirx * dirx + diry * diry) * prx_lo_rcp(o.max(np.abs(dirx), np.abs(diry)))
        len2x, len2y = 1.0 + (stretch - 1.0) * ln, 1.0 + -0.5 * ln
        lob = 0.5 + F32((1.0 / 4.0 - 0.04) - 0.5) * ln
        clp = prx_lo_rcp(lob)
        mn = o.min(o.min(c["f"], o.min(c["g"], c["j"])), c["k"])
        mx = o.max(o.max(c["f"], o.max(c["g"], c["j"])), c["k"])
        ac, aw, aw_abs = np.zeros((oh, ow, 3)), np.zeros((oh, ow)), np.zeros((oh, ow))
        for k, (ox, oy) in [("b", (0, -1)), ("c", (1, -1)), ("i", (-1, 1)), ("j", (0, 1)), ("f", (0, 0)), ("e", (-1, 0)), ("k", (1, 1)), ("l", (2, 1)), ("h", (2, 0)), ("g", (1, 0)),
                            ("o", (1, 2)), ("n", (0, 2))]:
            offx, offy = ox - ppx, oy - ppy
            vx, vy = (offx * dirx + offy * diry) * len2x, (offx * -diry + offy * dirx) * len2y
            d2 = o.min(vx * vx + vy * vy, clp)
            wb, wa = F32(2.0 / 5.0) * d2 - 1.0, lob * d2 - 1.0
            wb, wa = wb * wb, wa * wa
            wb = F32(25.0 / 16.0) * wb + F32(-(25.0 / 16.0 - 1.0))
            w = wb * wa
            ac, aw, aw_abs = ac + c[k] * w[..., None], aw + w, aw_abs + np.abs(w)
        pix = o.min(mx, o.max(mn, ac * (1.0 / aw)[..., None]))
        margin |= np.abs(aw) < 1e-3 * aw_abs          # (the lobes cancel: the quotient hangs on the rounding of the weights)
        nonfinite = sum((~np.isfinite(v).all(axis=-1)).astype(int) for v in c.values())
    return {"out": np.concatenate([pix, np.ones((oh, ow, 1))], axis=2), "margin": margin, "dont_care": o.mask, "line": line,
            "counts": {"zro": int(zro.sum()), "all_taps_nonfinite": int((nonfinite == 12).sum()), "rcp_of_zero": int((np.abs(L["g"] - L["f"]) + np.abs(L["f"] - L["e"]) == 0).sum())}}


def ref_rcas(input_bits, sharpness, mistake=None):
    t = Tex(half(input_bits))
    h, w = t.h, t.w
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    o = Open((h, w))
    with np.errstate(all="ignore"):
        sharp = 2.0 ** -F32(sharpness)
        b, d, e, f, hh = (t.load(x + dx, y + dy)[..., :3] for dx, dy in ((0, -1), (-1, 0), (0, 0), (1, 0), (0, 1)))
        if mistake == "diagonal_cross":
            b = t.load(x - 1, y - 1)[..., :3]
        mn4 = o.min(o.min(b, o.min(d, f)), hh)
        mx4 = o.max(o.max(b, o.max(d, f)), hh)
        hit_min = o.min(mn4, e) * (1.0 / (4.0 * mx4))
        hit_max = (1.0 - o.max(mx4, e)) * (1.0 / (4.0 * mn4 + -4.0))
        lobe3 = o.max(-hit_min, hit_max)
        lobe = o.max(-F32(0.25 - (1.0 / 16.0)), o.min(o.max(lobe3[..., 0], o.max(lobe3[..., 1], lobe3[..., 2])), 0.0)) * sharp
        rcp = prx_med_rcp(4.0 * lobe + 1.0)
        lb = lobe[..., None]
        pix = (lb * b + lb * d + lb * hh + lb * f + e) * rcp[..., None]
        nonfinite = sum((~np.isfinite(v).all(axis=-1)).astype(int) for v in (b, d, e, f, hh))
    return {"out": np.concatenate([pix, np.ones((h, w, 1))], axis=2), "margin": np.zeros((h, w), bool), "dont_care": o.mask,
            "counts": {"zero_times_inf": int(((mx4 == 0.0) & (mn4 == 0.0)).all(axis=-1).sum()), "peak_denominator_zero": int((mn4 == 1.0).all(axis=-1).sum()),
                       "cross_nonfinite": int((nonfinite == 5).sum()), "cross_touched": int((nonfinite > 0).sum())}}


def deviation_floored(want, got_bits, skip):
    """deviation_f16 with the unit floored at 2^-20 times the texel's largest component (at least 1): TAA, SMAA Tu4x and EASU sum up to a
    dozen terms of either sign whose size is that of the inputs, so their f32 sum carries up to 12 x 2^-24 of THAT size whatever is
    left of the result after cancellation - measured in ulps of a result near zero it has no bound"""
    got = half(got_bits)
    with np.errstate(all="ignore"):
        floor = 2.0 ** -20 * np.maximum(1.0, np.nanmax(np.where(np.isfinite(want), np.abs(want), 0.0), axis=2, keepdims=True))
        near_overflow = np.abs(np.abs(want) - 65520.0) < 1.0
        skip = skip[..., None] | near_overflow
        nan, inf, zero = np.isnan(want), np.abs(want) >= 65520.0, want == 0.0
        special_bad = (nan != np.isnan(got)) | (inf & ~nan & (got != np.sign(want) * np.inf)) | (~inf & ~nan & np.isinf(got)) | (zero & (np.abs(got) > floor))
        ordinary = ~nan & ~inf & ~skip & ~special_bad
        dev = np.where(ordinary, np.abs(got - want) / np.maximum(f16_ulp(want), floor), 0.0)
    return float(dev.max(initial=0.0)), (special_bad & ~skip).any(axis=2)


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import oracle_plugin

    p = oracle_plugin()
    p.set_scene(hk.load_cornell())
    return p.engine


def scatter(shape, r, keys, exact=()):
    """the texels a quad kernel stores, as (wanted plane, written mask, margin, dont_care) on the output grid; `exact`: keys whose texel
    is a copy of one input texel, whatever the thread's other texel hangs on"""
    h, w = shape
    want, written, margin, dont_care = np.zeros((h, w, 4)), np.zeros((h, w), bool), np.zeros((h, w), bool), np.zeros((h, w), bool)
    for key, (sx, sy) in zip(keys, r["at"]):
        ok = (sx >= 0) & (sy >= 0) & (sx < w) & (sy < h)
        want[sy[ok], sx[ok]] = r[key][ok]
        written[sy[ok], sx[ok]] = True
        if key not in exact:
            margin[sy[ok], sx[ok]], dont_care[sy[ok], sx[ok]] = r["margin"][ok], r["dont_care"][ok]
    return want, written, margin, dont_care


def scatter_mask(shape, at, mask):
    out = np.zeros(shape, bool)
    sx, sy = at
    ok = (sx >= 0) & (sy >= 0) & (sx < shape[1]) & (sy < shape[0])
    out[sy[ok], sx[ok]] = mask[ok]
    return out


def placed_on(planes, shape):
    """every mark of the set - on the G-buffer, the render, the TAA and the upscaled grid - carried to a plane of `shape` through the
    texel's uv"""
    h, w = shape
    out = np.zeros(shape, bool)
    for m in planes.placed.values():
        ys, xs = ((np.arange(h) + 0.5) / h * m.shape[0]).astype(int), ((np.arange(w) + 0.5) / w * m.shape[1]).astype(int)
        out |= m[np.ix_(ys, xs)]
    return out


def dispatches(e, planes, mistake=None, alone=False):
    """Run the tail on the oracle; per dispatch yield (kernel, reference output plane, written, margin, dont_care, counts, what the
    oracle wrote, `placed` on that grid).  alone: every pass on the WRITTEN planes, not on what the pass before it left."""
    b = planes.buffers
    PP.install_aa(e, planes)
    geometry = (b[F.BUF_POSITION], b[F.BUF_VELOCITY_UV], b[F.BUF_PREVIOUS_POSITION], b[F.BUF_PREVIOUS_VELOCITY_UV])
    clear = np.array([planes.frame.clear_color[i] for i in range(4)], dtype=np.float64)
    for pass_id in planes.passes:
        if alone:
            PP.install_aa(e, planes)
        if pass_id == F.PASS_SMAA_TU4X:
            r = ref_smaa(b[F.BUF_TONE_MAPPED], b[F.BUF_PREVIOUS_TONE_MAPPED], *geometry, b[F.BUF_INSTANCE_MATERIAL], planes.output_size, planes.frame.number, mistake)
            e.pass_run(pass_id)
            got = e.read(F.BUF_UPSCALE_OUTPUT)
            want, written, margin, dont_care = scatter(got.shape[:2], r, ("current", "previous"), exact=("current",))
            _EXEMPT[id(got)] = scatter_mask(got.shape[:2], r["at"][1], r["clip_margin"])
            yield "smaa_tu4x", want, written, margin, dont_care, r["counts"], got, placed_on(planes, got.shape[:2])
        elif pass_id == F.PASS_SMAA_TU4X_EXTRAPOLATE:
            r = ref_extrapolate(e.read(F.BUF_UPSCALE_OUTPUT), planes.render_size, mistake)
            e.pass_run(pass_id)
            got = e.read(F.BUF_UPSCALE_OUTPUT)
            want, written, margin, dont_care = scatter(got.shape[:2], r, ("x", "y"))
            yield "smaa_tu4x_extrapolate", want, written, margin, dont_care, r["counts"], got, placed_on(planes, got.shape[:2])
        elif pass_id == F.PASS_TAA_JASMINE:
            source = e.read(F.BUF_UPSCALE_OUTPUT) if planes.smaa else b[F.BUF_TONE_MAPPED]
            r = _TAA = ref_taa(source, b[F.BUF_PREVIOUS_TAA_OUTPUT], *geometry, planes.taa_size, planes.frame.upscale_ratio, clear, mistake)
            e.pass_run(pass_id)
            got = e.read(F.BUF_TAA_OUTPUT)
            _LINE[id(got)] = r["line"]
            yield "taa_jasmine", r["out"], np.ones(got.shape[:2], bool), r["margin"], r["dont_care"], r["counts"], got, placed_on(planes, got.shape[:2])
        elif pass_id == F.PASS_FSR_EASU:
            source = e.read(F.BUF_TAA_OUTPUT) if planes.taa == hk.Taa.Jasmine and not alone else b[F.BUF_TONE_MAPPED]
            if alone and planes.taa == hk.Taa.Jasmine:
                e.write(F.BUF_TAA_OUTPUT, b[F.BUF_TONE_MAPPED])
            r = ref_easu(source, planes.window_size, mistake)
            e.pass_run(pass_id)
            got = e.read(F.BUF_UPSCALE_OUTPUT)
            _LINE[id(got)] = r["line"]
            yield "fsr_easu", r["out"], np.ones(got.shape[:2], bool), r["margin"], r["dont_care"], r["counts"], got, placed_on(planes, got.shape[:2])
        elif pass_id == F.PASS_FSR_RCAS:
            r = ref_rcas(e.read(F.BUF_UPSCALE_OUTPUT), planes.upscale.sharpness_, mistake)
            e.pass_run(pass_id)
            got = e.read(F.BUF_UPSCALE_SHARPENED)
            yield "fsr_rcas", r["out"], np.ones(got.shape[:2], bool), r["margin"], r["dont_care"], r["counts"], got, placed_on(planes, got.shape[:2])


_LINE = {}          # the exactly aligned rows and columns of the dispatch last yielded (ref_easu, ref_taa), by the id of its output array
_EXEMPT = {}        # SMAA Tu4x: the pixels whose CLIP gathers at previous_output_uv - a texel centre of the G-buffer at ratio 2 by construction
exempted = {}       # ... how many placed texels that exemption covered, per kernel (reported)


def check(records, edge=False):
    worst, share, counts, problems = {}, {}, {}, []
    for kernel, want, written, margin, dont_care, c, got, placed in records:
        skip = margin | dont_care | ~written
        # (TAA alone sums Catmull-Rom weights of either sign and clips through a cancelling variance: its unit is floored; the others
        # are held in plain f16 ulps with exact zeros)
        dev, bad = deviation_floored(want, got, skip) if kernel == "taa_jasmine" else deviation_f16(want, got, skip)
        worst[kernel] = max(worst.get(kernel, 0.0), dev)
        if bad.any():
            ys, xs = np.nonzero(bad)
            problems.append(f"{kernel}: {int(bad.sum())} texels disagree on NaN / Inf / zero, first (x={xs[0]}, y={ys[0]}): {half(got)[ys[0], xs[0]]} vs {want[ys[0], xs[0]]}")
        if dev > BOUND_ULPS[kernel]:
            problems.append(f"{kernel}: {dev:.2f} ulp > {BOUND_ULPS[kernel]}")
        n = max(1, int(written.sum()))
        line = _LINE.pop(id(got), np.zeros_like(written))
        left_out = int(((margin | dont_care) & written & ~line).sum())
        share[kernel] = max(share.get(kernel, 0.0), left_out / n)
        if left_out > (int(np.ceil(EXCLUDED_CAP * n)) if edge else EXCLUDED_CAP * n):
            problems.append(f"{kernel}: {left_out} of {n} texels left out")
        exempt = _EXEMPT.pop(id(got), np.zeros_like(written)) | line
        exempted[kernel] = exempted.get(kernel, 0) + int((margin & placed & written & ~dont_care & exempt).sum())
        if (margin & placed & written & ~dont_care & ~exempt).any():      # (a texel left out as open anyway is not left out for the margin)
            problems.append(f"{kernel}: {int((margin & placed & written & ~dont_care & ~exempt).sum())} deliberately placed texels lie within rounding of a threshold")
        for k, v in c.items():
            counts[f"{kernel}.{k}"] = counts.get(f"{kernel}.{k}", 0) + v
    return worst, share, counts, problems


_measured, _shares = {}, {}

#: the branches a set claims, as least counts over the settings on the 130 x 17 render shape (both parities, chain and alone)
WANT = {
    "flat": {"taa_jasmine.clip_taken": 20, "smaa_tu4x.clip_taken": 5, "taa_jasmine.clip_pos_inf": 10, "taa_jasmine.clip_neg_inf": 10, "taa_jasmine.clip_zero_over_zero": 10,
             "taa_jasmine.clip_flat_residue": 10, "smaa_tu4x.clip_pos_inf": 5, "smaa_tu4x.clip_neg_inf": 5, "smaa_tu4x.clip_zero_over_zero": 5, "smaa_tu4x.clip_flat_residue": 5, "fsr_easu.zro": 50, "fsr_easu.rcp_of_zero": 50, "fsr_rcas.zero_times_inf": 4, "fsr_rcas.peak_denominator_zero": 4},
    "hdr": {"fsr_easu.all_taps_nonfinite": 1, "fsr_rcas.cross_nonfinite": 2, "smaa_tu4x_extrapolate.all_six_nonfinite": 2, "smaa_tu4x_extrapolate.loads_touched": 50, "fsr_rcas.cross_touched": 50},
    "reproject": {"taa_jasmine.boundary": 50, "smaa_tu4x.boundary": 600, "taa_jasmine.velocity": 50, "smaa_tu4x.velocity": 10},     # (584 of SMAA's are the quads that hang over the odd window)
    "depth": {"taa_jasmine.clear": 3200, "taa_jasmine.lone_depth": 5, "taa_jasmine.lone_slots": 150,     # (of 20 bias x corner slots in each of 16 runs)
               "taa_jasmine.depth": 100, "taa_jasmine.position": 100, "taa_jasmine.ties2": 1090, "taa_jasmine.ties3": 1,
              "taa_jasmine.ties4": 1, "smaa_tu4x.ties2": 553, "smaa_tu4x.depth": 50},      # (3104 clear pixels and 1084 / 552 double ties come with the fill)
    "instance": {"smaa_tu4x.instance": 10, "smaa_tu4x.step_1_no_miss": 10, "smaa_tu4x.step_1_ulp_miss": 10},
    "random": {"taa_jasmine.clip": 10, "taa_jasmine.clear": 10, "smaa_tu4x_extrapolate.loads_touched": 5, "fsr_rcas.cross_touched": 5},
}


def test_the_listed_flat_levels_are_what_the_search_finds():
    assert PP.negative_residue_levels(9) == PP.FLAT_LEVELS[9] and PP.negative_residue_levels(4, 1) == PP.FLAT_LEVELS[4] == []


@pytest.mark.parametrize("name", PP.AA_SETS)
def test_oracle_agrees_with_float64(oracle, name):
    problems, total = [], {}
    for shape in SHAPES + EDGE_SHAPES:
        for setting in PP.AA_SETTINGS:
            for parity in (2, 3):
                for alone in (False, True):
                    planes = PP.make_aa_planes(name, 7, PP.aa_window_for(shape, setting), setting, parity)
                    worst, share, counts, bad = check(dispatches(oracle, planes, alone=alone), edge=shape in EDGE_SHAPES)
                    problems += [f"{shape} {setting} f{parity}{' alone' if alone else ''}: {b}" for b in bad]
                    for k, v in worst.items():
                        _measured[k] = max(_measured.get(k, 0.0), v)
                    if shape in SHAPES:
                        for k, v in share.items():
                            _shares[k] = max(_shares.get(k, 0.0), v)
                    if shape == SHAPES[0]:
                        for k, v in counts.items():
                            total[k] = total.get(k, 0) + v
    print(name, "worst deviations so far", {k: round(v, 3) for k, v in _measured.items()}, "left-out shares so far", {k: round(v, 4) for k, v in _shares.items()}, "placed texels under a counted exemption so far", exempted,
          "branches", total)
    assert problems == []
    assert {k: total.get(k, 0) for k, v in WANT[name].items() if total.get(k, 0) < v} == {}, total


@pytest.mark.parametrize("mistake,name,setting,kernel", [("jitter_swapped", "depth", "smaa2_taa", "smaa_tu4x"), ("swapped_corners", "depth", "smaa2_taa", "smaa_tu4x"), ("weights_swapped", "reproject", "fsr10_taa", "taa_jasmine"),
                                                         ("transposed_blend", "random", "smaa2_taa", "smaa_tu4x_extrapolate"), ("mirrored_taps", "random", "fsr20", "fsr_easu"),
                                                         ("diagonal_cross", "random", "fsr20", "fsr_rcas")])
def test_the_comparison_notices_a_planted_mistake(oracle, mistake, name, setting, kernel):
    """Negative control: the restatement with SMAA's two jitters swapped, the corner offsets of nearest_velocity mirrored, the outer Catmull-Rom weights of TAA swapped, the extrapolated
    texel blended from the transposed neighbours, EASU's taps mirrored and RCAS's cross bent must each fail the comparison.  (A
    mistake AT a threshold - `>=` for `>` - cannot: the texels on a threshold are the margin; nor can swapped gather corners where
    the shader takes `any` of the four.)"""
    planes = PP.make_aa_planes(name, 7, PP.aa_window_for((130, 17), setting), setting, 3)
    *_, problems = check(dispatches(oracle, planes, mistake=mistake))
    assert [p for p in problems if p.startswith(kernel + ":") and ("ulp" in p or "disagree" in p)], problems


# ---------------------------------------------------------------- the shaders' own word: tests/golden/wgsl_aa_planes_*.npz
def shader_fixture_cases():
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import wgsl_pin

    return wgsl_pin


def replay_aa_planes(e, case):
    """tests/golden/wgsl_aa_planes_<case>.npz holds what the REFERENCE'S SHADERS - taa.wgsl, smaa.wgsl, FSR_Pass.glsl - wrote in every
    dispatch of the tail on the compact planes of `case` (tests/tools/wgsl_pin.py --aa-planes --write, run where the reference is at
    hand), and per plane a mask of the texels that rest on the contract's rule for a coordinate that is no number or outside the int
    range, which the shader text leaves open.  Drive engine `e` through the same dispatches and return the (dispatch, buffer) whose
    bytes differ from what the shader wrote outside that mask."""
    wgsl_pin = shader_fixture_cases()
    name, setting, render_size, frame_number = case
    data = np.load(wgsl_pin.aa_planes_fixture_path(*case))
    planes = PP.make_aa_planes(name, 7, PP.aa_window_for(render_size, setting), setting, frame_number, compact=True)
    PP.install_aa(e, planes)
    bad, seen = [], 0
    for index, pass_id in enumerate(planes.passes, start=1):
        e.pass_run(pass_id)
        for key in [k for k in data.files if k.startswith("d") and int(k[1:4]) == index]:
            got = e.read(int(key.split("buf")[1]))
            want = data[key].reshape(got.shape[0], got.shape[1], -1)
            differs = (got.view(np.uint8).reshape(want.shape) != want).any(axis=2) & ~data["mask_" + key].astype(bool)
            seen += 1
            if differs.any():
                bad.append((index, key, int(differs.sum())))
    assert seen == len(planes.passes) and len(data.files) == 2 * seen
    return bad


AA_PLANES_FIXTURES = shader_fixture_cases().AA_PLANES_FIXTURES
_ids = lambda c: f"{c[0]}-{c[1]}-f{c[3]}"


@pytest.mark.parametrize("case", AA_PLANES_FIXTURES, ids=_ids)
def test_oracle_equals_what_the_reference_shaders_wrote_on_the_planes(oracle, case):
    assert replay_aa_planes(oracle, case) == []


@pytest.mark.skipif(not shader_fixture_cases().reference_available(), reason="no reference checkout (HIKARI_REFERENCE_DIR)")
@pytest.mark.parametrize("case", AA_PLANES_FIXTURES, ids=_ids)
def test_reference_shaders_reproduce_the_oracle_on_the_planes(case):
    """taa.wgsl, smaa.wgsl and FSR_Pass.glsl themselves, executed dispatch by dispatch on the oracle's state: byte for byte, the texels
    under the mask included (there the runtime's samplers take the texel from the numeric contract)."""
    wgsl_pin = shader_fixture_cases()
    results = wgsl_pin.run_aa_planes(*case)
    assert results and [r for r in results if r["mismatch"]] == []
    data = np.load(wgsl_pin.aa_planes_fixture_path(*case))
    assert sorted(data.files) == sorted(wgsl_pin.run_aa_planes.recorded)
    assert all((data[k] == wgsl_pin.run_aa_planes.recorded[k]).all() for k in data.files)        # the committed fixture is what they write
