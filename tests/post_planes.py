"""Adversarial synthetic planes for the post chain (demodulation, the four a-trous levels, tone mapping).

Every other test feeds the denoiser frames rendered from a scene, which never hold the values its guard branches and fast paths
were written for.  `make_planes` builds the denoiser's INPUT planes directly - render / variance / albedo and the G-buffer planes
it reads - in the layouts `Engine.read` reports, and `install` writes them into an engine after `frame_begin`.  The frame uniform
carries nine DISTINCT kernel weights (a transposed kernel index changes the result) and four distinct clear-colour components.

Named sets - each places its special texels deterministically (a small image gets the ones that fall inside it) and fills the rest
from the seed:

  nonfinite   `nan_or_above_max` on centres and taps: NaN / +Inf / -Inf / 65504 in single components of render texels, isolated
              and as 3 x 3 blocks (after demodulation a centre whose eight level-3 taps are all rejected); demodulation's
              `variance > F32_MAX` skip and `max(variance, 0)`: NaN, +Inf, -1, 0, a denormal and 1e30 in the variance planes.
  thresholds  `albedo < 0.01` per component (0.01 -/+ one f16 ulp mixed within a texel); `depth < F32_EPSILON` (0, epsilon -/+ one
              f32 ulp, NaN); zero and anti-parallel stored normals (`normalize(0)`, `max(0, dot)`); instance ids differing by 0,
              0.25, 1 and 1 + ulp (`max(0, 1 - |di|)`); depth steps that leave `sum_w < 0.0001`, with and without a rejected centre.
  black       the wave-uniform black-channel shortcut of k_denoise, laid out against its 64 x 1 wave: channels 1 and 2 are +0 with
              alpha 1 (a nonzero `w` half) everywhere but for ONE lit texel at x = 63 in the middle row - at step s the wave of
              columns 64..127 in the rows s above and below has exactly one lane (63 + s) with exactly one lit tap - a `-0.0`
              texel, a NaN variance, a zero normal and a NaN depth under otherwise black spans.  `internal_variance` holds the
              plane a test may write over the demodulated variance for a NaN and a negative `lum_denominator` input.
  fireflies   the firefly clamp `lum > mean + 3 sigma`: isolated texels 10 .. 1e4 times a CONSTANT neighbourhood (ff_var about 0, of
              either sign after rounding) on the filtered channels 1, 2 and on channel 0 (not filtered), and a bright block under
              albedo 8 with a huge variance, which level 3 multiplies past the f16 range.
  random      dense seeded noise with a few percent of each special value.

`placed` marks (on the render grid) the texels a set placed deliberately.  A later change can add tone-mapped-plane sets for the
anti-aliasing tail here: `Planes.buffers` is an open mapping of buffer id -> array."""
import numpy as np

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F

SETS = ("nonfinite", "thresholds", "black", "fireflies", "random")
RENDER_WIDTHS, RENDER_HEIGHTS = (1, 63, 64, 65, 130), (1, 9, 17)
KERNEL = ((0.031, 0.109, 0.047), (0.127, 0.251, 0.139), (0.059, 0.151, 0.086))   # frame.kernel[column][row]: nine distinct weights, sum 1
CLEAR_COLOR = (0.125, 0.25, 0.5, 0.75)
F32_EPSILON = np.float32(1.1920929e-7)
H_NAN, H_INF, H_NINF, H_MAX, H_ONE, H_NZERO = 0x7E00, 0x7C00, 0xFC00, 0x7BFF, 0x3C00, 0x8000


def window_for(render_size, ratio):
    """The smallest window whose render image (ceil(window / ratio), light.rs:318-319) has `render_size`.  At ratio 1.5 that is
    not 1.5 times the render size, so no tap's jittered uv falls exactly between two G-buffer texels."""
    return tuple(int(np.floor((n - 1) * ratio)) + 1 for n in render_size)


def render_size_of(window_size, ratio):
    scale = np.float32(1.0) / np.float32(ratio)
    return tuple(int(np.ceil(scale * np.float32(n))) for n in window_size)


def f16_bits(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def pack_snorm8x4(n):
    b = np.floor(0.5 + 127.0 * np.clip(np.asarray(n, dtype=np.float64), -1.0, 1.0)).astype(np.int64) & 0xFF
    return (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24)).astype(np.uint32)


class Planes:
    def __init__(self, name, seed, window_size, ratio, channels, frame_number):
        self.name, self.seed, self.window_size, self.ratio, self.channels = name, seed, tuple(window_size), float(ratio), channels
        self.settings = hk.HikariSettings(indirect_bounces=2 if channels == 3 else 0, upscale=hk.Upscale.SmaaTu4x(ratio), clear_color=CLEAR_COLOR)
        self.frame = hk.frame_uniform(self.settings, frame_number)
        for c in range(3):
            for r in range(3):
                self.frame.kernel[c][r] = KERNEL[c][r]
        for i in range(4):
            self.frame.clear_color[i] = CLEAR_COLOR[i]
        self.buffers = {}        # buffer id -> array in Engine.read's layout
        self.internal_variance = None
        self.placed = None

    def __getitem__(self, key):
        return self.buffers[_BY_NAME[key]]


_BY_NAME = {"albedo": F.BUF_ALBEDO, "position": F.BUF_POSITION, "normal": F.BUF_NORMAL, "depth_gradient": F.BUF_DEPTH_GRADIENT,
            "instance_material": F.BUF_INSTANCE_MATERIAL}
for _i in range(3):
    _BY_NAME[f"render{_i}"], _BY_NAME[f"variance{_i}"] = F.BUF_RENDER0 + _i, F.BUF_VARIANCE0 + _i


def deferred_texel(p, x, y):
    """the G-buffer texel under render pixel (x, y): nearest texel of jittered_deferred_uv(coords_to_uv) (denoise.wgsl:37-41)"""
    (dw, dh), (rw, rh) = p.window_size, p.render_size
    sgn = -0.5 if p.frame.number % 2 == 0 else 0.5
    k = sgn * (float(np.float32(p.frame.upscale_ratio)) - 1.0)
    tx = int(np.clip(np.floor((x + 0.5) / rw * dw + k), 0, dw - 1))
    ty = int(np.clip(np.floor((y + 0.5) / rh * dh + k), 0, dh - 1))
    return tx, ty


def make_planes(name, seed, window_size, ratio, channels=3, frame_number=2, compact=False):
    """compact: the coordinates of the special texels, laid out for a 130 x 17 image, are scaled down to this image, so that a small
    one holds them all (the shader fixtures; on top of each other where they collide)"""
    assert name in SETS and channels in (2, 3)
    p = Planes(name, seed, window_size, ratio, channels, frame_number)
    rng = np.random.default_rng([seed, SETS.index(name)])
    dw, dh = p.window_size
    rw, rh = p.render_size = render_size_of(window_size, ratio)
    # (a special texel beyond the image goes to a spare last row / column that is cut off again: a small image gets the specials
    # that fall inside it, so their share of the image does not grow as the image shrinks)
    fit = (lambda x, y: (x * rw // 130, y * rh // 17)) if compact else (lambda x, y: (x, y))
    inside = lambda x, y: 0 <= x < rw and 0 <= y < rh
    at = lambda x, y: fit(x, y)[::-1] if inside(*fit(x, y)) else (rh, rw)                                  # render grid, [row, column]
    under = lambda x, y: deferred_texel(p, *fit(x, y))[::-1] if inside(*fit(x, y)) else (dh, dw)           # G-buffer grid, [row, column]

    # ---- the benign fill: one surface with a gentle depth ramp, two instances side by side, three normals, albedo 0.2 .. 0.9
    gx, gy = np.meshgrid(np.arange(dw), np.arange(dh))
    depth = (2.0 + 0.002 * gx + 0.003 * gy + 0.001 * rng.random((dh, dw))).astype(np.float32)
    position = np.zeros((dh, dw, 4), np.float32)
    position[..., :3] = rng.normal(size=(dh, dw, 3))
    position[..., 3] = depth
    dirs = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 0.3, 0.95]])
    n3 = dirs[(gx // 23 + gy // 11) % 3] + 0.02 * rng.normal(size=(dh, dw, 3))
    normal = pack_snorm8x4(np.concatenate([n3, np.zeros((dh, dw, 1))], axis=2))[..., None]
    gradient = (0.01 * rng.normal(size=(dh, dw, 2))).astype(np.float32)
    instance = np.zeros((dh, dw, 2), np.float32)
    instance[..., 0] = np.where(gx < (2 * dw) // 3, 1.5, 2.5)
    instance[..., 1] = 0.5
    albedo = np.ones((dh, dw, 4), np.float32)
    albedo[..., :3] = 0.2 + 0.7 * rng.random((dh, dw, 3))
    background = (gx >= dw - max(1, dw // 10)) & (gy < dh // 2) if dw > 8 else np.zeros((dh, dw), bool)     # a block without geometry
    position[background, 3] = 0.0
    render = np.ones((3, rh, rw, 4), np.float32)
    render[..., :3] = 0.05 + 1.5 * rng.random((3, rh, rw, 3))
    variance = (0.5 * rng.random((3, rh, rw, 1))).astype(np.float32)
    ivar = (0.3 * rng.random((rh, rw, 1))).astype(np.float32)
    spare = lambda a, axis: np.pad(a, [(0, 1) if k in (axis, axis + 1) else (0, 0) for k in range(a.ndim)])
    position, normal, gradient, instance, albedo, ivar = (spare(a, 0) for a in (position, normal, gradient, instance, albedo, ivar))
    render, variance = spare(render, 1), spare(variance, 1)
    render_bits = f16_bits(render)
    albedo_bits = f16_bits(albedo)
    placed = np.zeros((rh + 1, rw + 1), bool)

    def texel(ch, x, y, comp, bits):
        render_bits[(ch,) + at(x, y) + (comp,)] = bits
        placed[at(x, y)] = True

    if name == "nonfinite":
        for x, y, ch, comp, bits in ([(5, 3, 1, 0, H_NAN), (20, 2, 0, 1, H_INF), (33, 5, 2, 2, H_NINF), (40, 6, 0, 0, H_MAX),
                                                    (12, 7, 2, 1, H_NAN), (50, 1, 1, 2, H_INF), (58, 8, 1, 1, H_MAX), (90, 4, 0, 2, H_NAN)]):
            texel(ch, x, y, comp, bits)
        for ch, (x0, y0, bits) in enumerate([(25, 10, H_NAN), (70, 3, H_INF), (100, 11, H_NAN)]):     # 3 x 3 blocks: a rejected centre whose eight step-1 taps are rejected
            for ox in (-1, 0, 1):
                for oy in (-1, 0, 1):
                    texel(ch, x0 + ox, y0 + oy, (ox + oy) % 3, bits)
        # All eight taps of (x0 + 8, 8) rejected at every step 8, 4, 2, 1 - for the level that is run straight on the demodulated plane
        # (a level fed by the one before it sees the finite values that one wrote).  Channel 0: the centre rejected as well (sum_w = 0,
        # the fallback); channels 1 and 2: a good centre with ff_count = 0.
        texel(0, 16, 8, 1, H_INF)
        for ch, x0 in enumerate((8, 44, 80)):
            for step in (8, 4, 2, 1):
                for ox, oy in ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
                    texel(ch, x0 + 8 + ox * step, 8 + oy * step, 0, H_INF)
        specials = np.array([np.nan, np.inf, -1.0, 0.0, 1e-40, 1e30], np.float32)
        for ch in range(3):
            for k in range(18):
                x, y = 3 + 7 * k + ch, (2 * k + ch + 1) % 17      # (the NaN ones, k = 0, 6, 12, off row 0: one is three left-out texels of a 64 x 1 image)
                variance[(ch,) + at(x, y)] = specials[k % 6]
                placed[at(x, y)] = True
    elif name == "thresholds":
        lo, hi = np.uint16(0x211E), np.uint16(0x211F)    # the f16 values around 0.01: 0.0099945 and 0.0100021
        for x, y, bits in ([(4, 2, (lo, hi, lo)), (17, 5, (hi, lo, hi)), (30, 7, (lo, lo, lo)), (45, 3, (hi, hi, hi)), (66, 9, (lo, hi, hi)),
                                          (2, 0, (0, hi, lo)), (90, 12, (hi, 0, H_NZERO))]):
            albedo_bits[under(x, y)][:3] = bits
            placed[at(x, y)] = True
        eps = F32_EPSILON
        for x, y, d in [(9, 1, 0.0), (11, 1, np.nextafter(eps, np.float32(0))), (13, 1, eps), (15, 1, np.nextafter(eps, np.float32(1))), (22, 12, np.nan),
                        (52, 10, np.float32(-1.0)), (77, 2, np.float32(np.inf))]:
            position[under(x, y)][3] = d
            placed[at(x, y)] = True
        for x, y, n in [(27, 4, (0, 0, 0)), (28, 4, (0, 0, -1.0)), (61, 9, (-0.6, 0, -0.8)), (101, 13, (0, 0, 0))]:
            normal[under(x, y)] = pack_snorm8x4(np.array(n + (0,), dtype=np.float64))
            placed[at(x, y)] = True
        for x, y, i in [(36, 2, 1.5), (37, 2, 1.75), (38, 2, 2.5), (39, 2, np.nextafter(np.float32(2.5), np.float32(3))), (36, 11, 1.25), (84, 5, 2.0)]:
            instance[under(x, y)][0] = i
            placed[at(x, y)] = True
        # sum_w < 0.0001: a texel alone at its depth under a flat gradient - every tap's w_depth underflows - with its centre rejected
        # (sum_w = 0 exactly) and, at a smaller step, with the taps' weights tiny but not zero and the centre rejected too
        for x, y, d in [(48, 6, 100.0), (49, 12, 2.3), (110, 8, 100.0), (20, 14, 2.25)]:
            ty, tx = under(x, y)
            position[ty, tx, 3] = np.float32(d) + position[ty, tx, 3] - np.float32(2.0)
            gradient[ty, tx] = 0.0
            for ch in range(3):
                render_bits[(ch,) + at(x, y) + (ch,)] = H_NAN
            placed[at(x, y)] = True
    elif name == "black":
        for ch in (1, 2):
            render_bits[ch, ..., :3] = 0
            render_bits[ch, ..., 3] = H_ONE
            xl, yl = 63, (rh // 2 + ch - 1)
            for comp in range(3):
                texel(ch, xl, yl, comp, f16_bits(0.75 + 0.5 * comp))
            texel(ch, 10, 2 + ch, 0, H_NZERO)
            texel(ch, 129, 5, 1, H_NZERO)
            variance[(ch,) + at(100, 3)] = np.nan
            placed[at(100, 3)] = True
        normal[under(110, 5)] = 0
        position[under(90, 14)][3] = np.nan
        placed[at(110, 5)] = placed[at(90, 14)] = True
        ivar[at(100, 3)] = np.nan
        ivar[at(101, 11)] = -0.25
        ivar[at(20, 13)] = np.inf
    elif name == "fireflies":
        level = np.array([0.3, 0.5, 0.2], np.float32)
        for ch in range(3):                       # a flat fill (30 % noise: ff_var stays clearly positive through the levels) ...
            render[ch, ..., :3] = level * (1.0 + ch) * (1.0 + 0.3 * rng.random((rh + 1, rw + 1, 1)))
            render[(ch,) + at(105, 3)][:3] = level * (1.0 + ch) * 200.0       # ... but for one firefly in an exactly constant patch (not `placed`:
            for x in range(103, 108):                                         # rounding decides the sign of its ff_var)
                for y in range(1, 6):
                    if (x, y) != (105, 3):
                        render[(ch,) + at(x, y)][:3] = level * (1.0 + ch)
        render_bits = f16_bits(render)
        albedo[..., :3] = 0.5                     # constant: the demodulated neighbourhoods are constant too
        albedo_bits = f16_bits(albedo)
        variance[...] = 0.01
        for x, y, gain in ([(6, 3, 10.0), (19, 7, 100.0), (31, 12, 1000.0), (43, 4, 10000.0), (57, 9, 30.0), (70, 14, 300.0), (95, 6, 3000.0), (120, 10, 50.0)]):
            for ch in range(3):
                render_bits[(ch,) + at(x, y)][:3] = f16_bits(np.minimum(level * (1.0 + ch) * gain, 60000.0))
                placed[at(x, y)] = True
        for x in range(74, 81):                   # a bright block under albedo 8 whose neighbours sit under albedo 1: level 3 multiplies past 65504
            for y in range(1, 8):
                ty, tx = under(x, y)
                centre = (x, y) == (77, 4)
                albedo_bits[ty, tx, :3] = f16_bits(8.0 if centre else 1.0)
                render_bits[(0,) + at(x, y)][:3] = f16_bits(60000.0)      # (channel 0 only: on a filtered channel the constant block's
                variance[(0,) + at(x, y)] = 1e30                          # ff_var is 0 but for rounding)
                placed[at(x, y)] = True
    position, normal, gradient, instance, albedo_bits = (a[:dh, :dw] for a in (position, normal, gradient, instance, albedo_bits))
    ivar, placed = ivar[:rh, :rw], placed[:rh, :rw]
    render_bits, variance = render_bits[:, :rh, :rw], variance[:, :rh, :rw]
    if name == "random":
        area = rw * rh

        def some(shape, count):
            """`count` distinct random positions of an array of `shape`, as a mask (a COUNT, not a rate: what WGSL leaves open under one
            texel spreads over the nine pixels that tap it, and the comparison may leave out 2 % of an image at the most)"""
            m = np.zeros(int(np.prod(shape)), bool)
            m[rng.choice(m.size, size=min(count, m.size), replace=False)] = True
            return m.reshape(shape)

        for bits in (H_INF, H_MAX, 0, H_NZERO):          # (-Inf passes every test and spreads NaN: the `nonfinite` set places it)
            render_bits[..., :3][rng.random((3, rh, rw, 3)) < 0.004] = bits
        render_bits[..., :3][some((3, rh, rw, 3), area // 120)] = H_NAN
        for v in (np.inf, -1.0, 1e30, 0.0):
            variance[rng.random(variance.shape) < 0.02] = v
        variance[some(variance.shape, area // 400)] = np.nan
        m = rng.random((dh, dw)) < 0.03
        position[m, 3] = rng.choice(np.array([0.0, 1e-8, 1e-7, 50.0], np.float32), size=int(m.sum()))
        position[some((dh, dw), area // 1200), 3] = np.nan
        normal[some((dh, dw), area // 1200)] = 0
        albedo_bits[..., :3][rng.random((dh, dw, 3)) < 0.03] = 0x211E
        albedo_bits[..., :3][rng.random((dh, dw, 3)) < 0.03] = 0x211F
        render_bits[..., 3][rng.random((3, rh, rw)) < 0.03] = f16_bits(-1.0)
        render_bits[..., 3][rng.random((3, rh, rw)) < 0.01] = H_NAN
        render_bits[..., 3][rng.random((3, rh, rw)) < 0.03] = 0
        instance[rng.random((dh, dw)) < 0.03, 0] += 0.25

    for ch in range(3):
        p.buffers[F.BUF_RENDER0 + ch] = np.ascontiguousarray(render_bits[ch])
        p.buffers[F.BUF_VARIANCE0 + ch] = np.ascontiguousarray(variance[ch])
    p.buffers.update({F.BUF_ALBEDO: albedo_bits, F.BUF_POSITION: position, F.BUF_NORMAL: normal, F.BUF_DEPTH_GRADIENT: gradient,
                      F.BUF_INSTANCE_MATERIAL: instance})
    p.buffers = {buf: np.ascontiguousarray(a) for buf, a in p.buffers.items()}
    p.internal_variance, p.placed = np.ascontiguousarray(ivar), placed
    return p


def install(engine, planes, resize=True):
    """hk_resize (if the size changed), hk_frame_begin with the planes' frame uniform, then hk_write_buffer of every plane."""
    size = planes.window_size + (planes.ratio,)
    if resize and getattr(engine, "_post_planes_size", None) != size:
        engine.resize(*size)
        engine._post_planes_size = size
    camera = hk.cornell_camera(*planes.window_size)
    engine.frame_begin(planes.frame, camera.view_uniform(), camera.previous_view_uniform(None), hk.lights_uniform())
    for buf, array in planes.buffers.items():
        engine.write(buf, array)          # (hk_write_buffer refuses a size that is not the buffer's)


# ------------------------------------------------------------------------------------------------------------------------------
# The anti-aliasing / upscale tail: k_smaa_tu4x, k_smaa_tu4x_extrapolate, k_taa_jasmine, k_fsr_easu, k_fsr_rcas
# ------------------------------------------------------------------------------------------------------------------------------
"""Plane sets for the tail (`make_aa_planes`).  The five kernels read the tone-mapped image of this frame and the last one, the
last TAA output, both position and velocity planes and the instance ids; `upscale_output` is filled as well, for the passes that
are run alone on a written input (the extrapolate pass, RCAS, and TAA under SMAA Tu4x).  Coordinates below are RENDER pixels of a
130 x 17 image; a special goes to the texel of each plane that lies under that pixel's centre, blocks scale with the plane.

  flat       exactly constant 3 x 3 patches of render pixels (3 x 3 for TAA, 2 x 2 for SMAA and more) at 0, 1, 0.5, at the two first
             levels of FLAT_LEVELS and at one coloured constant, with the history equal to the patch (`v_clip / e_clip` is 0 / 0) or
             coloured above / below it in every YCoCg component (+Inf, -Inf), inside blocks where every reprojection test misses
             (so the clip runs); one image carries five of the 17 patches, which ones rotates with the setting and the parity.
             `moment_2 / n - mean * mean` rounds below zero in f32 at the FLAT_LEVELS (found by `negative_residue_levels`, a search
             over the f16 greys); EASU sees a flat input (`zro`, and `prx_lo_rcp(0)`), RCAS a flat 0 (`0 * (1 / 0)`) and a flat 1
             (`4 * mn4 - 4 == 0`).
  hdr        NaN, +Inf, -Inf, 65504, -0.0, negative values and values above 1 in single components of the current and the history
             colour planes, isolated and as a block of 2 x 2 render pixels (at least 4 x 4 texels of the upscaled planes: every tap of RCAS's cross and
             of the extrapolate pass's six loads non-finite for a pixel inside) and, under FSR1, of 3 x 3 in the image's corner (EASU's 12 taps); alphas other than 1.
  reproject  velocities (the fill moves by 0.3 output texels: at 0 every gather of the previous frame sits on a texel centre): 0, one
             and half an output texel, the values whose `fract(v / (2 texel))` is 0, 0.25 and 0.5 and the same
             negated, a `previous_uv` of exactly 0 and 1 and one f32 ulp outside, +-3, 1e9, 3e38, +-Inf, NaN;
             `|velocity - previous_velocity|` at 0.00005 and 0.0001, one ulp either side.
  depth      previous depths 0, negative, NaN, +Inf and a denormal; current depth 0; a depth ratio of 0.95 and one ulp either side;
             a position distance of 0.5 and one ulp either side; a block whose 20 gathered previous depths are all <= 0 under a
             current depth of 0 (the clear colour), with ONE positive texel in a second such block (every bias and gather corner
             sees it alone from some pixel); corner depths of `nearest_velocity` with two, three and four ties at the maximum, the
             centre equal to the maximum, NaN among the corners.
  instance   stripes of instance ids that differ by 0, by 1.0 exactly and by 1 + ulp, the upper half of each with a depth-ratio
             miss at the same taps and the lower half without, under a velocity miss.
  random     dense seeded noise with a small COUNT of each special."""
AA_SETS = ("flat", "hdr", "reproject", "depth", "instance", "random")
#: name -> (upscale, taa): SMAA Tu4x at ratio 2 (with `window_for`, an odd window: 2 x render > output, store_loose cuts the quad)
#: and at ratio 1, FSR1 at 1.0 / 1.5 / 2.0 with TAA at the scaled size, TAA on and off, sharpness 0, 0.2 and 2
AA_SETTINGS = {
    "smaa2_taa": (hk.Upscale.SmaaTu4x(2.0), hk.Taa.Jasmine),
    "smaa2": (hk.Upscale.SmaaTu4x(2.0), hk.Taa.NONE),
    "smaa1_taa": (hk.Upscale.SmaaTu4x(1.0), hk.Taa.Jasmine),
    "fsr10_taa": (hk.Upscale.Fsr1(1.0, 0.2), hk.Taa.Jasmine),
    "fsr15_taa": (hk.Upscale.Fsr1(1.5, 2.0), hk.Taa.Jasmine),
    "fsr20": (hk.Upscale.Fsr1(2.0, 0.0), hk.Taa.NONE),
}
FSR_SIZES = (1, 15, 16, 17, 33, 130)       # output widths / heights for the 16 x 16 tiles of the two FSR kernels


def _ycocg_y32(c):
    """y of RGB_to_YCoCg for a grey c, in f32 and in the shaders' order"""
    c = np.float32(c)
    return np.float32(np.float32(c / np.float32(4.0)) + np.float32(c / np.float32(2.0))) + np.float32(c / np.float32(4.0))


def negative_residue_levels(n, count=4):
    """f16 greys in (0, 1) for which `moment_2 / n - mean * mean` over n equal samples is NEGATIVE in f32 (sums left to right, as
    the shaders write them): sqrt of it is NaN, and the clip box has NaN corners on an exactly constant neighbourhood."""
    found = []
    for bits in range(0x3000, 0x3C00, 7):          # 0.125 .. 1, every 7th f16
        y = _ycocg_y32(np.uint16(bits).view(np.float16))
        m1, m2, sq = np.float32(0), np.float32(0), np.float32(y * y)
        for _ in range(n):
            m1, m2 = np.float32(m1 + y), np.float32(m2 + sq)
        mean = np.float32(m1 / np.float32(n))
        if np.float32(np.float32(m2 / np.float32(n)) - np.float32(mean * mean)) < 0:
            found.append(bits)
            if len(found) == count:
                break
    return found


#: the greys `negative_residue_levels` finds (f16 bits: 0.1668, 0.1685, 0.1703, 0.172), for the nine samples of TAA; the test module
#: asserts that the search still gives this list.  For the four samples of SMAA Tu4x there are none, whatever the colour: 4 s and
#: 4 (s * s) are exact in f32 and so are their quarters, so `moment_2 / 4 - mean * mean` is s * s - s * s = 0 exactly.
FLAT_LEVELS = {9: [0x3157, 0x3165, 0x3173, 0x3181], 4: []}


class AaPlanes:
    def __init__(self, name, seed, window_size, setting, frame_number):
        self.name, self.seed, self.window_size, self.setting = name, seed, tuple(window_size), setting
        self.upscale, self.taa = AA_SETTINGS[setting]
        self.ratio = float(self.upscale.ratio())
        self.settings = hk.HikariSettings(indirect_bounces=1, upscale=self.upscale, taa=self.taa, clear_color=CLEAR_COLOR)
        self.frame = hk.frame_uniform(self.settings, frame_number)
        for i in range(4):
            self.frame.clear_color[i] = CLEAR_COLOR[i]
        w, h = self.window_size
        self.render_size = render_size_of(window_size, self.ratio)
        scale2 = np.float32(np.float32(1.0) / np.float32(self.ratio)) * np.float32(2.0)
        self.smaa = self.upscale.kind == F.UPSCALE_SMAA_TU4X
        self.upscaled_size = (int(np.ceil(np.float32(w) * scale2)), int(np.ceil(np.float32(h) * scale2)))     # UW x UH of hk_resize
        self.output_size = self.upscaled_size if self.smaa else self.window_size             # upscale_output
        self.taa_size = self.upscaled_size if self.smaa else self.render_size               # taa_output, previous_taa_output
        self.buffers, self.placed = {}, {}

    @property
    def passes(self):
        """the dispatches of the tail for these settings, in PostProcessNode::run's order"""
        p = [F.PASS_SMAA_TU4X, F.PASS_SMAA_TU4X_EXTRAPOLATE] if self.smaa else []
        p += [F.PASS_TAA_JASMINE] if self.taa == hk.Taa.Jasmine else []
        return p + ([] if self.smaa else [F.PASS_FSR_EASU, F.PASS_FSR_RCAS])


def aa_window_for(shape, setting):
    """the window for a RENDER shape (the 64 x 4 row kernels) under a setting"""
    return window_for(shape, AA_SETTINGS[setting][0].ratio())


def make_aa_planes(name, seed, window_size, setting, frame_number=2, compact=False):
    assert name in AA_SETS
    p = AaPlanes(name, seed, window_size, setting, frame_number)
    rng = np.random.default_rng([seed, 100 + AA_SETS.index(name)])
    (dw, dh), (rw, rh), (tw, th), (ow, oh) = p.window_size, p.render_size, p.taa_size, p.output_size
    lw, lh = (rw, rh) if compact else (130, 17)            # the layout the coordinates below are written for

    class Grid:
        """one plane size: where the render pixel (x, y) of the layout lies in it, as [row, column]; outside the image -> the spare"""
        def __init__(self, w, h):
            self.w, self.h = w, h
            self.placed = np.zeros((h + 1, w + 1), bool)

        def fit(self, x, y):
            if compact:
                x, y = x * rw // 130, y * rh // 17
            return x, y

        def at(self, x, y):
            x, y = self.fit(x, y)
            if not (0 <= x < rw and 0 <= y < rh):
                return self.h, self.w
            return min(int((y + 0.5) / rh * self.h), self.h - 1), min(int((x + 0.5) / rw * self.w), self.w - 1)

        def block(self, x, y, size):
            """`size` render pixels square with its corner at (x, y), in this plane's texels (at least size texels)"""
            r, c = self.at(x, y)
            if r == self.h:
                return slice(self.h, self.h + 1), slice(self.w, self.w + 1)
            nr, nc = max(size, int(np.ceil(size * self.h / rh))), max(size, int(np.ceil(size * self.w / rw)))
            return slice(r, min(r + nr, self.h)), slice(c, min(c + nc, self.w))

        def mark(self, where):
            self.placed[where] = True

    G, R, T, O = Grid(dw, dh), Grid(rw, rh), Grid(tw, th), Grid(ow, oh)
    spare = lambda a: np.pad(a, [(0, 1), (0, 1)] + [(0, 0)] * (a.ndim - 2))

    # ---- the benign fill.  Every reprojection test holds (velocities differ from texel to texel by less than both thresholds): the
    # clip runs where a set places a block in which every test misses (`still(miss=True)`: previous depth doubled, previous position
    # 1 away, previous velocity 0.01 off) and nowhere else - at ratio 2 the clip's own gathers sit on texel centres, where rounding
    # picks the footprint, and a comparison may leave out 2 %.  The last 10 % of the upper half has no geometry now or before (the
    # clear colour)
    gx, gy = np.meshgrid(np.arange(dw), np.arange(dh))
    missing = np.zeros((dh, dw), bool)
    background = (gx >= dw - max(1, dw // 10)) & (gy < dh // 2) if dw > 8 else np.zeros((dh, dw), bool)
    depth = (2.0 + 0.002 * gx + 0.003 * gy).astype(np.float32)
    position = np.zeros((dh, dw, 4), np.float32)
    position[..., 0], position[..., 1], position[..., 2] = 0.01 * gx, 0.01 * gy, 0.005 * (gx + gy)
    position[..., 3] = depth
    previous_position = position + np.float32(0.002) * rng.random((dh, dw, 4)).astype(np.float32)
    previous_position[missing, 3] *= np.float32(2.0)
    previous_position[missing, 0] += np.float32(1.0)
    position[background, 3] = 0.0
    previous_position[background, 3] = 0.0
    velocity = np.zeros((dh, dw, 4), np.float32)
    velocity[..., :2] = (0.0002 + 0.00002 * (rng.random((dh, dw, 2)) - 0.5)).astype(np.float32)
    # (half the columns move by about 0.2 G-buffer texels exactly: a velocity of 0 puts every gather of the previous frame on a texel centre,
    # where rounding picks the footprint - the `reproject` set places it, the fill keeps off it)
    steady = np.array([0.1871 / dw, 0.2137 / dh], np.float32)      # (in G-buffer texels, no simple fraction - the gathers stay off the texel centres at every ratio - and short of the quarter texel between the first SMAA sample and the border)
    velocity[(gx // 16) % 2 == 0, :2] = steady
    previous_velocity = velocity.copy()
    previous_velocity[..., :2] += (2e-6 * rng.random((dh, dw, 2))).astype(np.float32)
    previous_velocity[missing, 0] += np.float32(0.01)
    instance = np.zeros((dh, dw, 2), np.float32)
    instance[..., 0] = np.where(gx < dw // 3, 1.0, 3.0)
    instance[..., 1] = 0.5

    def colour(grid, alpha_noise):
        c = np.ones((grid.h, grid.w, 4), np.float32)
        c[..., :3] = 0.05 + 0.9 * rng.random((grid.h, grid.w, 3))
        if alpha_noise:
            c[..., 3] = 0.25 + 0.75 * rng.random((grid.h, grid.w))
        return spare(f16_bits(c))

    position, previous_position, velocity, previous_velocity, instance = (spare(a) for a in (position, previous_position, velocity, previous_velocity, instance))
    tone, prev_tone, prev_taa, upscaled = colour(R, name == "hdr"), colour(R, False), colour(T, False), colour(O, name == "hdr")
    current, history = [(tone, R), (upscaled, O)], [(prev_tone, R), (prev_taa, T)]
    one_ulp = lambda v, towards: np.nextafter(np.float32(v), np.float32(towards))

    # One special texel costs a comparison a dozen or more pixels (every kernel here has a footprint), and a comparison may leave out
    # 2 % of a dispatch: an image carries every sixth of a set's blocks (`turns`) - which, rotates with the setting and the parity, so that
    # every block meets every kernel under one SMAA Tu4x and one FSR1 setting
    # (an image under 2000 render pixels: every twelfth - its 2 % are a dozen pixels)
    turns = 6 if rw * rh >= 2000 else 12
    variant = (2 * list(AA_SETTINGS).index(setting) + frame_number % 2) % turns
    mine = lambda k: k % turns == variant

    def still(x, y, size, miss):
        """a block that moves by `steady` (the reprojected uv lies 0.3 texels from the pixel's own) with every test missing or holding"""
        b = G.block(x, y, size)
        velocity[b] = 0.0
        velocity[b + (slice(0, 2),)] = steady
        previous_velocity[b] = velocity[b]
        if miss:
            previous_velocity[b + (0,)] = steady[0] + np.float32(0.01)
        previous_position[b] = position[b]
        if miss:
            previous_position[b + (3,)] = position[b + (3,)] * np.float32(2.0)
            previous_position[b + (0,)] = position[b + (0,)] + np.float32(1.0)
        return b

    if name == "flat":
        # (level, history): the history equal to the patch (0 / 0 in the clip), or coloured above / below it in every YCoCg component
        # (+Inf / -Inf).  A comparison may leave out 2 % of a dispatch and at ratio 2 every clipped pixel of SMAA Tu4x sits within
        # rounding of a gather boundary, so one image carries five of the patches (three under 2000 render pixels): which, rotates with the setting and the parity
        greys = [0x0000, H_ONE, 0x3800] + FLAT_LEVELS[9][:2]
        patches = [(bits, hist) for bits in greys for hist in ("equal", "above", "below")] + [((0.75, 0.25, 0.5), "equal"), ((0.75, 0.25, 0.5), "above")]
        variant = 2 * list(AA_SETTINGS).index(setting) + frame_number % 2
        chosen = [patches[(variant + 4 * k) % len(patches)] for k in range(4 if turns == 6 else 2)]
        chosen = chosen[:1] + [patches[(variant * 5 + 1) % len(patches)]] + chosen[1:]          # (the second lies where every test holds: no clip)
        for k, (level, hist) in enumerate(chosen):
            x, y = 6 + 24 * k, 2 + 3 * (k % 4)
            still(x, y, 3, miss=k != 1)
            rgbv = np.array(level if isinstance(level, tuple) else [float(np.uint16(level).view(np.float16))] * 3, np.float32)
            past = {"equal": rgbv, "above": rgbv * np.float32([1.5, 2.0, 1.25]) + np.float32([0.125, 0.25, 0.0625]), "below": rgbv * np.float32([0.5, 0.25, 0.75])}[hist]
            for planes, value in ((current, rgbv), (history, past)):
                for a, grid in planes:
                    b = grid.block(x, y, 3)
                    a[b + (slice(0, 3),)] = f16_bits(value)
                    grid.mark(b)
    elif name == "hdr":
        # (few: one non-finite texel reaches 16 outputs of EASU and a dozen of TAA, and a comparison may leave out 2 % of a dispatch)
        singles = {"current": [(5, 3, 0, H_NAN), (33, 5, 2, 0xC100), (58, 8, 1, 0x4500), (84, 12, 0, H_MAX), (104, 2, 1, H_NZERO), (12, 14, 2, 0xBC00), (70, 15, 3, 0x3800)],
                   "history": [(20, 2, 1, H_INF), (50, 10, 0, H_NAN), (95, 13, 2, H_NINF), (110, 6, 1, 0x4000), (40, 6, 0, 0xB800), (33, 5, 2, 0x4500)]}
        for planes, key in ((current, "current"), (history, "history")):
            for k, (x, y, comp, bits) in enumerate(singles[key]):
                if not (mine(k) or (key == "current" and turns == 6 and mine(k + 3))):
                    continue
                for a, grid in planes:
                    where = grid.at(x, y)
                    a[where + (comp,)] = bits
                    if key == "current":      # (a history texel: the Catmull-Rom taps that sit on texel centres next to it hang on rounding - not `placed`)
                        grid.mark(where)
        # (FSR1: the block sits in the image's corner, 3 x 3 render pixels - with clamp-to-edge all 12 taps of EASU's first output pixels
        # are non-finite, and the block reaches a quarter of the outputs it would reach in the middle)
        corner = [(0, 0, 3, H_NAN if frame_number % 2 else H_INF)] if not p.smaa and rw * rh >= 1000 and (mine(0) or mine(3)) else []
        for planes, blocks in ((current, corner + ([(25, 9, 2, H_NAN if frame_number % 2 else H_INF)] if turns == 6 and (mine(2) or mine(4) or (p.smaa and mine(0))) else [])), (history, [(76, 3, 2, H_NAN)] if mine(5) else [])):
            for x, y, size, bits in blocks:
                for a, grid in planes:
                    b = grid.block(x, y, size)
                    a[b + (slice(0, 3),)] = bits
                    if planes is current:      # (history: as the single texels above)
                        grid.mark(b)
    elif name == "reproject":
        tx, ty = np.float32(1.0) / np.float32(tw if p.taa == hk.Taa.Jasmine else ow), np.float32(1.0) / np.float32(th if p.taa == hk.Taa.Jasmine else oh)
        values = [(0.0, 0.0), (tx, ty), (tx / 2, ty / 2), (-tx, 0.0), (0.0, -ty / 2), (2 * tx, 2 * ty), (tx * 5 / 2, -ty * 5 / 2), (-tx / 2, ty), (3 * tx, -ty),
                  (3.0, 0.0), (0.0, -3.0), (-3.0, 3.0), (1e9, 0.0), (0.0, -1e9), (3e38, 3e38), (-3e38, 0.0), (np.inf, 0.0), (0.0, -np.inf), (np.inf, np.inf),
                  (np.nan, 0.0), (0.0, np.nan), (np.nan, np.nan), (-np.inf, np.nan)]
        for k, v in enumerate(values):
            if not mine(k) or (rw * rh < 1000 and not np.isfinite(v).all()):      # (under 1000 pixels one NaN velocity alone costs EASU over 2 %)
                continue
            x, y = 2 + 8 * (k % 15), 1 + 6 * (k // 15) + (k % 3)
            b = still(x, y, 2 if turns == 6 or np.isfinite(v).all() else 1, miss=k % 2 == 0)      # (no number: through TAA and EASU one texel reaches two dozen outputs)
            velocity[b + (slice(0, 2),)] = np.array(v, np.float32)
            # (none of these is `placed`: a whole or half number of texels - +-3 is one at every width - puts the gathers on texel centres
            # and the nearest taps on boundaries by construction, 1e9 leaves f32 no fraction, and what no number reaches is open)
        # a previous_uv of exactly 0 and 1, and one ulp outside: the velocity is the uv of the block's own first pixel (minus 1), nudged
        for k, (edge, nudge) in enumerate([(0.0, 0), (0.0, 1), (1.0, 0), (1.0, -1)]):
            if not mine(k + 1):
                continue
            x, y = 4 + 30 * k, 14
            b = still(x, y, 2, miss=False)
            r, c = G.at(x, y)
            if r < dh:
                grid_w, grid_h = (tw, th) if p.taa == hk.Taa.Jasmine else (ow, oh)
                px, py = int((c + 0.5) / dw * grid_w), int((r + 0.5) / dh * grid_h)
                u, v = (np.float32(px) + np.float32(0.5)) / np.float32(grid_w), (np.float32(py) + np.float32(0.5)) / np.float32(grid_h)
                vu, vv = np.float32(u - np.float32(edge)), np.float32(v - np.float32(edge))
                if nudge:
                    vu, vv = one_ulp(vu, nudge * np.inf), one_ulp(vv, nudge * np.inf)
                velocity[b + (slice(0, 2),)] = np.array([vu, vv], np.float32)      # (on the boundary test's threshold by design: not `placed`)
        for k, d in enumerate([0.00005, 0.0001]):
            for j, towards in enumerate((None, 0.0, 1.0)):
                if not mine(3 * k + j):
                    continue
                x, y = 70 + 8 * j, 8 + 4 * k
                b = still(x, y, 2, miss=True)
                dv = np.float32(d) if towards is None else one_ulp(d, towards)
                velocity[b] = 0.0                     # (0 - dv is exact; within rounding of the threshold by design: not `placed`)
                previous_velocity[b] = 0.0
                previous_velocity[b + (0,)] = dv
    elif name == "depth":
        specials = [0.0, -1.0, np.nan, np.inf, 1e-40, -0.0]
        for k, d in enumerate(specials):
            for j, plane in enumerate((previous_position, previous_position, position)):
                if not mine(k + 2 * j):
                    continue
                x, y = 3 + 9 * k, 1 + 5 * j
                b = still(x, y, 4, miss=False) if j else G.at(x, y)
                if j == 2 and d != 0.0:
                    continue
                plane[b + (3,)] = d
                G.mark(b)
        ratio = np.float32(0.95)
        for k, r in enumerate([ratio, one_ulp(ratio, 0.0), one_ulp(ratio, 1.0)]):
            if not mine(2 * k):
                continue
            b = still(60 + 8 * k, 2, 2, miss=False)
            previous_position[b + (3,)] = 2.0
            position[b + (3,)] = np.float32(2.0) * r
            previous_velocity[b + (0,)] = steady[0] + np.float32(0.01)         # (a velocity miss, so that the depth test decides)
            previous_position[b + (0,)] = position[b + (0,)] + np.float32(1.0)      # (on the threshold by design: not `placed`)
        for k, dist in enumerate([np.float32(0.5), one_ulp(0.5, 0.0), one_ulp(0.5, 1.0)]):
            if not mine(2 * k + 1):
                continue
            b = still(60 + 8 * k, 8, 2, miss=False)
            position[b + (slice(0, 3),)] = 0.0
            previous_position[b + (slice(0, 3),)] = np.array([dist, 0.0, 0.0], np.float32)
            previous_position[b + (3,)] = position[b + (3,)] * np.float32(2.0)
            previous_velocity[b + (0,)] = steady[0] + np.float32(0.01)      # (on the threshold by design: not `placed`)
        for k, lone in enumerate((False, True)):        # 20 gathered previous depths <= 0 under a current depth of 0; then ONE positive texel
            b = still(86 + 14 * k, 1, 12, miss=False)
            position[b + (3,)] = 0.0
            previous_position[b + (3,)] = np.where(rng.random(previous_position[b + (3,)].shape) < 0.5, 0.0, -1.0)
            if lone and b[0].stop - b[0].start > 2:
                previous_position[(b[0].start + b[0].stop) // 2, (b[1].start + b[1].stop) // 2, 3] = 1.5
            G.mark(b)
        # corner depths of nearest_velocity around a centre of 1.0: (x+ y+, x- y+, x+ y-, x- y-)
        # (in this order: the two slots of SMAA Tu4x at ratio 2 with TAA - where TAA's input texel is the G-buffer's - get four, three and two ties)
        patterns = [(3, 3, 3, 3), (3, 3, 3, 1), (1, 1, 1, 1), (0.5, 1, 0.5, 0.5), (np.nan, 3, 1, 1), (np.nan, np.nan, np.nan, np.nan), (3, 3, 1, 1), (3, 1, 1, 3), (3, np.nan, 3, 1)]
        for k, corners in enumerate(patterns):
            if not mine(k):
                continue
            r, c = G.at(4 + 9 * k, 13)
            if 1 <= r < dh - 1 and 1 <= c < dw - 1:
                position[r - 1:r + 2, c - 1:c + 2, 3] = 1.0
                for (oy, ox), d in zip(((1, 1), (1, -1), (-1, 1), (-1, -1)), corners):
                    position[r + oy, c + ox, 3] = d
                nine = np.arange(9).reshape(3, 3)      # nine distinct velocities, so that the offset shows - each an odd fraction of a G-buffer texel, off every centre and boundary
                velocity[r - 1:r + 2, c - 1:c + 2, 0], velocity[r - 1:r + 2, c - 1:c + 2, 1] = (0.1871 + 0.0731 * nine) / dw, (0.2137 + 0.0611 * nine) / dh
                previous_velocity[r - 1:r + 2, c - 1:c + 2, :2] = velocity[r - 1:r + 2, c - 1:c + 2, :2]
                G.mark((slice(r - 1, r + 2), slice(c - 1, c + 2)))
    elif name == "instance":
        for k, step in enumerate([np.float32(0.0), np.float32(1.0), one_ulp(2.0, 3.0) - np.float32(1.0)]):
            for j, miss in enumerate((True, False)):
                if not mine(2 * k + j):
                    continue
                x, y = 4 + 18 * k, 1 + 8 * j
                b = still(x, y, 4, miss=False)
                previous_velocity[b + (0,)] = steady[0] + np.float32(0.01)                              # a velocity miss: instance_miss / depth_miss decide
                if miss:
                    previous_position[b + (3,)] = position[b + (3,)] * np.float32(2.0)
                ids = np.where((np.arange(b[1].start, b[1].stop) - b[1].start) % 4 < 2, np.float32(1.0), np.float32(1.0) + step)
                instance[b + (0,)] = ids[None, :]
                G.mark(b)
    position, previous_position, velocity, previous_velocity, instance = (a[:dh, :dw] for a in (position, previous_position, velocity, previous_velocity, instance))
    tone, prev_tone, prev_taa, upscaled = tone[:rh, :rw], prev_tone[:rh, :rw], prev_taa[:th, :tw], upscaled[:oh, :ow]
    if name == "random":
        area = dw * dh

        def some(shape, count):
            m = np.zeros(int(np.prod(shape)), bool)
            m[rng.choice(m.size, size=min(count, m.size), replace=False)] = True
            return m.reshape(shape)

        # (COUNTS, and few: one special texel reaches a dozen outputs of every kernel and a comparison may leave out 2 %.  Every plane
        # gets `count` specials, each of a kind drawn from the plane's list - over the settings, parities and shapes every kind turns up)
        count = 0 if area < 600 else max(1, area // 4000)          # (an image 1 wide or 1 high: its 2 % are no texel at all)

        def sprinkle(plane, kinds, index=None):
            if not compact and area < 8000 and rng.random() > area / 8000:      # (a small image: not every plane gets one; the compact fixtures: every plane)
                return
            for _ in range(count):
                where = some(plane.shape[:2], 1)
                kind = kinds[int(rng.integers(len(kinds)))]
                if index is None:
                    plane[where, int(rng.integers(3))] = kind
                else:
                    plane[where, index] = kind

        for a in (tone, prev_tone, prev_taa, upscaled):
            sprinkle(a, (H_NAN, H_INF, H_NINF, H_MAX, 0, H_NZERO, 0xBC00, 0x4200))
            a[..., 3][some(a[..., 3].shape, count)] = f16_bits(0.5)
        for plane in (position, previous_position):
            sprinkle(plane, (0.0, -1.0, np.nan, np.inf, 1e-40, 50.0), 3)
            plane[some((dh, dw), 4 * count), 0] += np.float32(0.75)
        for plane in (velocity, previous_velocity):
            sprinkle(plane, (0.0, 1.0 / max(tw, 1), 0.5 / max(tw, 1), -3.0, 3.0, 1e9, 3e38, np.inf, -np.inf, np.nan, 0.00005, 0.0001), int(rng.integers(2)))
        instance[some((dh, dw), 8 * count), 0] += np.float32(1.0)
        instance[some((dh, dw), 8 * count), 0] += np.float32(2.5)
    p.buffers = {F.BUF_TONE_MAPPED: tone, F.BUF_PREVIOUS_TONE_MAPPED: prev_tone, F.BUF_PREVIOUS_TAA_OUTPUT: prev_taa, F.BUF_UPSCALE_OUTPUT: upscaled,
                 F.BUF_POSITION: position, F.BUF_PREVIOUS_POSITION: previous_position, F.BUF_VELOCITY_UV: velocity,
                 F.BUF_PREVIOUS_VELOCITY_UV: previous_velocity, F.BUF_INSTANCE_MATERIAL: instance}
    p.buffers = {buf: np.ascontiguousarray(a) for buf, a in p.buffers.items()}
    p.placed = {"window": G.placed[:dh, :dw], "render": R.placed[:rh, :rw], "taa": T.placed[:th, :tw], "output": O.placed[:oh, :ow]}
    return p


def install_aa(engine, planes, resize=True):
    """hk_resize (if the size changed), the view options (the sizes of the upscale planes follow the upscale kind), hk_frame_begin,
    then every plane - the previous frame's after hk_frame_begin too, which is what decides which plane `PREVIOUS_*` names - and
    zeros in the planes the tail writes."""
    size = planes.window_size + (planes.ratio,)
    if resize and getattr(engine, "_post_planes_size", None) != size:
        engine.resize(*size)
        engine._post_planes_size = size
    engine.set_view_options(planes.taa, planes.upscale.kind, planes.upscale.sharpness_)
    camera = hk.cornell_camera(*planes.window_size)
    engine.frame_begin(planes.frame, camera.view_uniform(), camera.previous_view_uniform(None), hk.lights_uniform())
    for buf, array in planes.buffers.items():
        engine.write(buf, array)
    for buf in (F.BUF_TAA_OUTPUT, F.BUF_UPSCALE_SHARPENED):
        engine.write(buf, np.zeros_like(engine.read(buf)))


# ------------------------------------------------------------------------------------------------------------------------------
# spatial_reuse: k_spatial_reuse<emissive or indirect, plain or windowed>
# ------------------------------------------------------------------------------------------------------------------------------
"""Plane sets for ONE spatial_reuse dispatch (`make_spatial_planes`): the three G-buffer planes the pass reads (position with the
depth in .w, instance_material, velocity_uv), the channel's `current` and `previous_spatial` reservoirs as 64-byte records
(`pack_records` mirrors pack_reservoir, light.wgsl:111-136) and a sentinel fill of everything the pass writes or must leave alone.
Coordinates below are RENDER pixels of a 70 x 45 image; `compact` scales them into a small one.  Material ids stay inside the table of
`spatial_scene()`; the frame uniform comes from hk.frame_uniform.

  terraces    the benign fill: depths on the lattice 2 + k / 64 in terraces a few texels wide (every depth ratio within 3 % of 1, every
              march comparison an exact tie or off by 1 / 384 and more), normals from three directions 15, 40 and 55 degrees apart,
              samples one unit in front of or behind their surface, counts 1 .. 20, radiance 0.05 .. 3, a background block.
  depths      the centre depth 0 and F32_EPSILON -/+ one ulp; NaN, +Inf, negative and denormal depths at a centre, at a neighbour and
              under a march step; depth ratios of 0.9 and 1.1 -/+ one ulp on both sides; a one-texel occluder at each march step of
              the longest and of the shortest marched tap; an occluder 1e-5 -/+ one ulp above the interpolated depth; taps that land on
              background texels (depth / 0) and, at ratios above 1, taps at the border whose jittered texel lies outside the plane.
  records     neighbour counts 0, denormal, F32_EPSILON -/+ ulp, 4, 5, 65504, +Inf, NaN; sums that cross max_spatial_reuse_count
              exactly, by one, not at all; w / w_sum / w2_sum of 0, 65504, Inf, NaN; radiance +0, -0, NaN, 65504; normals at the
              0.866 threshold -/+ one snorm step, zero and anti-parallel; samples on the visible position, edge-on and behind; the
              Jacobian flag with edge-on / averted sample normals, near and far; lifetimes around the limit and at 254; the `random`
              sums that put some tap's angle nearest to 0, 1/4, 1/2 and 3/4 of a turn.
  history     previous_uv exactly 0, one ulp under 1, exactly 1, negative, NaN, +-Inf, 1e9; a history record that passes, a zero one.
  background  all-background wave tiles, tiles with one geometry pixel in a corner lane, a whole workgroup of background next to one of
              geometry, a NaN-depth pixel as a tile's only non-background lane.
  random      dense seeded noise with a few percent of each special, on a depth plane in which every texel differs."""
SPATIAL_SETS = ("terraces", "depths", "records", "history", "background", "random")
SPATIAL_WIDTHS, SPATIAL_HEIGHTS = (1, 8, 17, 49, 70), (1, 17, 45)
SPATIAL_COUNTS, SPATIAL_LIFETIMES, SPATIAL_RATIOS = (4, 100, 800), (0.0, 1.0, 7.0), (1.0, 1.5, 2.0)
T_SLOT, S_SLOT = (0, 2, 6), (4, 4, 8)              # light.rs:518-546, as make_light_targets and wgsl_pin.Pinner.reservoirs
SENTINEL_U32, SENTINEL_F32, SENTINEL_F16 = 0xC3A5C3A5, np.float32(-12345.5), 0x5BCD
SPATIAL_NORMALS = np.array([[0.0, 0.0, 1.0], [np.sin(np.radians(15.0)), 0.0, np.cos(np.radians(15.0))], [-np.sin(np.radians(40.0)), 0.0, np.cos(np.radians(40.0))]])
#: (base colour, metallic, perceptual roughness): roughness either side of the 0.089 clamp, metallic 0 and 1
SPATIAL_MATERIALS = [((0.8, 0.7, 0.6), 0.0, 0.5), ((0.2, 0.9, 0.3), 1.0, 0.05), ((0.9, 0.1, 0.1), 0.0, 0.089), ((0.3, 0.3, 0.95), 1.0, 0.09),
                     ((1.0, 1.0, 1.0), 0.0, 1.0), ((0.05, 0.5, 0.7), 0.0, 0.0885)]
_f32 = np.float32


def spatial_scene():
    """one triangle per material (the pass traces nothing): six materials distinct in colour, metallic and roughness, no textures"""
    b = hk.SceneBuilder()
    mesh = b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1]] * 3, [[0, 0], [1, 0], [0, 1]])
    for k, (colour, metallic, roughness) in enumerate(SPATIAL_MATERIALS):
        m = b.add_material(hk.standard_material(colour + (1.0,), perceptual_roughness=roughness, metallic=metallic, reflectance=0.3 + 0.1 * k))
        t = np.eye(4, dtype=np.float32)
        t[3, 0] = 3.0 * k
        b.add_instance(mesh, m, t)
    return b.finish()


def _hash(value):
    """utils.wgsl:15-24"""
    s = value & 0xFFFFFFFF
    s ^= 2747636419
    s = (s * 2654435769) & 0xFFFFFFFF
    s ^= s >> 16
    s = (s * 2654435769) & 0xFFFFFFFF
    s ^= s >> 16
    s = (s * 2654435769) & 0xFFFFFFFF
    return s


def random_float(value):
    return _f32(_f32(_hash(value)) / _f32(4294967295.0))


class Records:
    """reservoirs of one buffer on a grid, field by field, in the units of their storage: f16 BITS for count / w / w_sum / w2_sum and
    the radiance, unorm16 CODES for random, f32 for the positions and the instance, snorm8 BYTES (int8) for the normals, the lifetime
    as a number 0 .. 254 (byte = lifetime - 127) and the flag byte (127: the sample has a Jacobian)"""

    def __init__(self, h, w):
        self.count, self.w, self.w_sum, self.w2_sum = (np.zeros((h, w), np.uint16) for _ in range(4))
        self.radiance, self.random = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 4), np.uint16)
        self.visible_position, self.sample_position = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 3), np.float32)
        self.visible_instance = np.zeros((h, w), np.float32)
        self.visible_normal, self.sample_normal = np.zeros((h, w, 3), np.int8), np.zeros((h, w, 3), np.int8)
        self.lifetime, self.jacobian_flag = np.full((h, w), 127, np.int16), np.zeros((h, w), np.int8)

    def crop(self, h, w):
        out = Records(0, 0)
        for k, v in vars(self).items():
            setattr(out, k, np.ascontiguousarray(v[:h, :w]))
        return out

    def zero(self, where):
        for k, v in vars(self).items():
            v[where] = 127 if k == "lifetime" else 0


def pack_records(r):
    """[h, w, 16] u32: PackedReservoir (light.wgsl:35-43) word for word"""
    h, w = r.count.shape
    out = np.zeros((h, w, 16), np.uint32)
    u = lambda lo, hi: lo.astype(np.uint32) | (hi.astype(np.uint32) << 16)
    out[..., 0], out[..., 1] = u(r.radiance[..., 0], r.radiance[..., 1]), u(r.radiance[..., 2], r.radiance[..., 3])
    out[..., 2], out[..., 3] = u(r.random[..., 0], r.random[..., 1]), u(r.random[..., 2], r.random[..., 3])
    out[..., 4:8] = r.visible_position.view(np.uint32)
    out[..., 8:11] = r.sample_position.view(np.uint32)
    out[..., 11] = r.visible_instance.view(np.uint32)
    b = lambda n, last: (n[..., 0].astype(np.uint8).astype(np.uint32) | (n[..., 1].astype(np.uint8).astype(np.uint32) << 8) |
                         (n[..., 2].astype(np.uint8).astype(np.uint32) << 16) | (last.astype(np.uint8).astype(np.uint32) << 24))
    out[..., 12] = b(r.visible_normal, (r.lifetime - 127).astype(np.int8))
    out[..., 13] = b(r.sample_normal, r.jacobian_flag)
    out[..., 14], out[..., 15] = u(r.count, r.w), u(r.w_sum, r.w2_sum)
    return out


def snorm8(n):
    return np.floor(0.5 + 127.0 * np.clip(np.asarray(n, dtype=np.float64), -1.0, 1.0)).astype(np.int8)


class SpatialPlanes:
    def __init__(self, name, seed, window_size, ratio, channel, frame_number, max_count, max_lifetime):
        self.name, self.seed, self.window_size, self.ratio, self.channel = name, seed, tuple(window_size), float(ratio), channel
        self.settings = hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SmaaTu4x(ratio), max_spatial_reuse_count=max_count,
                                          max_reservoir_lifetime=max_lifetime, emissive_spatial_reuse=True)
        self.frame = hk.frame_uniform(self.settings, frame_number)
        self.render_size = render_size_of(window_size, ratio)
        cur = frame_number % 2
        prev = 1 - cur
        self.slots = {"previous": F.BUF_RESERVOIR0 + cur + T_SLOT[channel], "current": F.BUF_RESERVOIR0 + prev + T_SLOT[channel],
                      "previous_spatial": F.BUF_RESERVOIR0 + cur + S_SLOT[channel], "spatial": F.BUF_RESERVOIR0 + prev + S_SLOT[channel]}
        self.pass_id = F.PASS_EMISSIVE_SPATIAL_REUSE if channel == 1 else F.PASS_INDIRECT_SPATIAL_REUSE
        self.buffers, self.placed = {}, None
        self.current = self.previous_spatial = None          # Records on the render grid

    @property
    def outputs(self):
        """what the pass writes"""
        return {"spatial": self.slots["spatial"], "variance": F.BUF_VARIANCE0 + self.channel, "render": F.BUF_RENDER0 + self.channel}

    @property
    def untouched(self):
        """what it reads or must leave alone"""
        return {"current": self.slots["current"], "previous_spatial": self.slots["previous_spatial"], "previous": self.slots["previous"],
                "position": F.BUF_POSITION, "instance_material": F.BUF_INSTANCE_MATERIAL, "velocity_uv": F.BUF_VELOCITY_UV}


def spatial_deferred(p, u, v):
    """jittered_deferred_coords (light.wgsl:1007-1017) of a uv in f32, unclamped: (column, row) of the G-buffer texel"""
    dw, dh = p.window_size
    sgn = _f32(-0.25) if p.frame.number % 2 == 0 else _f32(0.25)
    ratio = _f32(_f32(p.frame.upscale_ratio) - _f32(1.0))
    ju = _f32(_f32(u) + _f32(_f32(sgn * _f32(_f32(1.0) / _f32(dw))) * ratio))
    jv = _f32(_f32(v) + _f32(_f32(sgn * _f32(_f32(1.0) / _f32(dh))) * ratio))
    return int(np.trunc(_f32(ju * _f32(dw)))), int(np.trunc(_f32(jv * _f32(dh))))


def spatial_texel(p, x, y):
    rw, rh = p.render_size
    return spatial_deferred(p, _f32(_f32(x + 0.5) / _f32(rw)), _f32(_f32(y + 0.5) / _f32(rh)))


def spatial_tap(p, x, y, i, random_sum=0.0):
    """tap i (1 ..) of render pixel (x, y) whose record's random components sum to `random_sum`: (sample pixel, [march texels]) as the
    shader places them (light.wgsl:1568-1576, 1609-1618), in f32 with numpy's cos and sin - for PLACING specials, no reference"""
    count, reach = (8, 10.0) if p.channel == 1 else (16, 20.0)
    rw, rh = p.render_size
    turn = _f32(_f32(_f32(_f32(i) * _f32(1.618033989)) + _f32(random_sum)) + random_float(p.frame.number))
    angle = _f32(_f32(6.283185307) * _f32(turn - np.floor(turn)))
    radius = _f32(np.sqrt(_f32(_f32(i) / _f32(count))) * _f32(reach))
    ox, oy = _f32(radius * np.cos(angle, dtype=np.float32)), _f32(radius * np.sin(angle, dtype=np.float32))
    sx, sy = int(np.trunc(_f32(ox + _f32(x)))), int(np.trunc(_f32(oy + _f32(y))))
    interval = max(_f32(1.0), _f32(radius / _f32(5.0)))
    n = int(_f32(radius / interval))
    length = _f32(np.sqrt(_f32(ox * ox + oy * oy)))
    u, v = _f32(_f32(x + 0.5) / _f32(rw)), _f32(_f32(y + 0.5) / _f32(rh))
    march = []
    for j in range(1, n + 1):
        d = _f32(_f32(j) * interval)
        march.append(spatial_deferred(p, _f32(u + _f32(_f32(d * _f32(ox / length)) / _f32(rw))), _f32(v + _f32(_f32(d * _f32(oy / length)) / _f32(rh)))))
    return (sx, sy), march


def quarter_turn_randoms(frame_number, count=16):
    """for each of 0, 1/4, 1/2, 3/4 of a turn: the unorm16 code c whose decoded value c / 65535 (the other three components 0) puts
    fract(i * golden + random + random_float(frame)) nearest to it for some tap i - a search over the codes (f32, the shader's order)"""
    codes = np.arange(65536, dtype=np.float32) / _f32(65535.0)
    found = []
    for target in (0.0, 0.25, 0.5, 0.75):
        best = None
        for i in range(1, count + 1):
            t = (_f32(_f32(i) * _f32(1.618033989)) + codes).astype(np.float32) + random_float(frame_number)
            fr = (t - np.floor(t)).astype(np.float32)
            d = np.abs(fr.astype(np.float64) - target)
            if target == 0.0:
                d = np.minimum(d, 1.0 - fr.astype(np.float64))
            k = int(np.argmin(d))
            if best is None or d[k] < best[0]:
                best = (float(d[k]), k, i)
        found.append((best[1], best[2]))
    return found


def make_spatial_planes(name, seed, render_size, ratio, channel, frame_number=2, max_count=800, max_lifetime=0.0, compact=False):
    """One spatial_reuse dispatch of `channel` (1 emissive, 2 indirect) at `render_size`, the window being window_for(render_size, ratio)."""
    assert name in SPATIAL_SETS and channel in (1, 2)
    p = SpatialPlanes(name, seed, window_for(render_size, ratio), ratio, channel, frame_number, max_count, max_lifetime)
    assert p.render_size == tuple(render_size)
    rng = np.random.default_rng([seed, 200 + SPATIAL_SETS.index(name), channel])
    (dw, dh), (rw, rh) = p.window_size, p.render_size
    fit = (lambda x, y: (x * rw // 70, y * rh // 45)) if compact else (lambda x, y: (x, y))
    inside = lambda x, y: 0 <= x < rw and 0 <= y < rh
    placed = np.zeros((rh + 1, rw + 1), bool)

    def at(x, y, mark=True):
        """render grid [row, column] of a layout pixel (the spare row / column when it falls outside)"""
        x, y = fit(x, y)
        if not inside(x, y):
            return rh, rw
        if mark:
            placed[y, x] = True
        return y, x

    def under(x, y, fitted=False):
        """G-buffer [row, column] under a layout pixel"""
        if not fitted:
            x, y = fit(x, y)
        if not inside(x, y):
            return dh, dw
        tx, ty = spatial_texel(p, x, y)
        return (ty, tx) if 0 <= tx < dw and 0 <= ty < dh else (dh, dw)

    # ---- the G-buffer: terraces (or, for `random`, a depth that differs in every texel) facing the camera of cornell_camera
    gx, gy = np.meshgrid(np.arange(dw + 1), np.arange(dh + 1))
    terrace = (gx // 5 + gy // 4) % 4
    depth = (2.0 + terrace / 64.0).astype(np.float32)
    if name == "random":
        depth = (2.0 + 0.1 * rng.permutation((dw + 1) * (dh + 1)).reshape(dh + 1, dw + 1) / ((dw + 1) * (dh + 1))).astype(np.float32)
    position = np.zeros((dh + 1, dw + 1, 4), np.float32)
    position[..., 0], position[..., 1], position[..., 2] = 0.02 * (gx - dw / 2), 1.0 + 0.02 * (dh / 2 - gy), 4.0 - depth
    position[..., 3] = depth
    background = (gx >= dw - max(1, dw // 10)) & (gy < dh // 2) if dw > 8 else np.zeros((dh + 1, dw + 1), bool)
    instance = np.zeros((dh + 1, dw + 1, 2), np.float32)
    instance[..., 0] = (gx // 9 + gy // 7) % len(SPATIAL_MATERIALS)
    instance[..., 1] = instance[..., 0]                               # material id = instance id: inside the table
    velocity = np.zeros((dh + 1, dw + 1, 4), np.float32)
    velocity[..., 2:] = rng.random((dh + 1, dw + 1, 2))
    # (history: every third column block looks one render pixel to the left, the rest at the pixel itself)
    velocity[..., 0] = np.where((gx // 6) % 3 == 1, _f32(1.0) / _f32(rw), _f32(0.0))

    # ---- the records of `current` and `previous_spatial`, on the render grid
    ry, rx = np.meshgrid(np.arange(rh + 1), np.arange(rw + 1), indexing="ij")
    tex_of = np.array([[under(x, y, fitted=True) for x in range(rw)] + [(dh, dw)] for y in range(rh)] + [[(dh, dw)] * (rw + 1)])
    ty_, tx_ = tex_of[..., 0], tex_of[..., 1]

    def fill():
        r = Records(rh + 1, rw + 1)
        shape = (rh + 1, rw + 1)
        r.count[...] = f16_bits(rng.integers(1, 21, shape))
        r.w[...] = f16_bits(0.1 + 1.9 * rng.random(shape))
        r.w_sum[...] = f16_bits(0.5 + 9.5 * rng.random(shape))
        r.w2_sum[...] = f16_bits(0.5 + 49.5 * rng.random(shape))
        r.radiance[..., :3] = f16_bits(0.05 + 2.95 * rng.random(shape + (3,)))
        r.radiance[..., 3] = np.where(rng.random(shape) < 0.85, H_ONE, 0)          # input_radiance.a: lit, or the ambient miss
        r.random[...] = rng.integers(0, 65536, shape + (4,))
        r.visible_position[...] = position[ty_, tx_]
        which = (rx // 11 + ry // 6) % 3
        normal = SPATIAL_NORMALS[which]
        r.visible_normal[...] = snorm8(normal)
        front = rng.random(shape) < 0.8                                             # the sample: one unit in front of the surface, or behind it
        lateral = 0.3 * (rng.random(shape + (3,)) - 0.5)
        r.sample_position[...] = (r.visible_position[..., :3] + np.where(front[..., None], 1.0, -1.0) * normal + lateral).astype(np.float32)
        r.sample_normal[...] = snorm8(-normal + 0.2 * (rng.random(shape + (3,)) - 0.5))
        r.jacobian_flag[...] = np.where(rng.random(shape) < 0.5, 127, 0)
        life = rng.integers(0, 11, shape)
        r.lifetime[...] = life + (life >= 7)                                          # 0 .. 6, 8 .. 11: never AT the limit of 7 (127 * (1 + b / 127) is not 7 in f32)
        r.visible_instance[...] = instance[ty_, tx_, 0]
        return r

    cur, hist = fill(), fill()
    hist.zero(rng.random((rh + 1, rw + 1)) < 0.1)                                     # a tenth of the history is empty
    one_ulp = lambda v, towards: np.nextafter(_f32(v), _f32(towards))
    n_taps = 8 if channel == 1 else 16

    def centre(x, y):
        """a centre pixel whose tap pattern is known: random = 0, a long history refusal left to the fill"""
        cur.random[at(x, y)] = 0
        return fit(x, y)

    def neighbour(x, y, i):
        """the render pixel [row, column] tap i of layout pixel (x, y) lands on and the G-buffer texels of its march, or None"""
        fx, fy = fit(x, y)
        (sx, sy), march = spatial_tap(p, fx, fy, i, 0.0)
        if not (inside(fx, fy) and inside(sx, sy)):
            return None
        placed[sy, sx] = True
        return (sy, sx), under(sx, sy, fitted=True), [(ty, tx) if 0 <= tx < dw and 0 <= ty < dh else (dh, dw) for tx, ty in march]

    def flat_all():
        """terrace 0 everywhere, one normal, every sample in front: every tap merges unless the set says otherwise (a special is not
        to depend on which terrace or normal the fill gave its surroundings)"""
        position[..., 2:] = 2.0
        cur.visible_position[...] = position[ty_, tx_]
        cur.visible_normal[...] = snorm8(SPATIAL_NORMALS[0])
        cur.sample_position[...] = cur.visible_position[..., :3] + _f32([0.05, 0.02, 1.0])

    eps = F32_EPSILON
    if name == "depths":
        flat_all()
        specials = [0.0, np.nextafter(eps, _f32(0)), eps, np.nextafter(eps, _f32(1)), np.nan, np.inf, -1.0, 1e-40]
        for k, d in enumerate(specials):                       # at a centre
            position[under(3 + 8 * k, 2)][3] = d
            at(3 + 8 * k, 2)
        for k, d in enumerate(specials[4:] + [0.0]):           # at a neighbour (tap 3) and under a march step of tap 12 / 6 only
            x, y = 8 + 12 * k, 12
            centre(x, y)
            n = neighbour(x, y, 3)
            if n:
                position[n[1]][3] = d
            m = neighbour(x, y, n_taps - 4)
            if m and len(m[2]) > 2:
                position[m[2][2]][3] = d
        ratios = [_f32(0.9), one_ulp(0.9, 0), one_ulp(0.9, 1), _f32(1.1), one_ulp(1.1, 0), one_ulp(1.1, 2)]
        for k, q in enumerate(ratios):                         # depth / sample_depth around 0.9 and 1.1: sample_depth = 2, depth = 2 q (exact)
            x, y = 6 + 11 * k, 24
            centre(x, y)
            position[under(x, y)][3] = _f32(2.0) * q
            cur.visible_position[at(x, y)][3] = _f32(2.0) * q
        for k in range(5):                                     # a one-texel occluder at march step k of the longest tap and of the shortest marched tap
            for row, i in ((34, n_taps), (40, 1)):
                x, y = 5 + 13 * k, row
                centre(x, y)
                n = neighbour(x, y, i)
                if n and k < len(n[2]):
                    position[n[2][k]][3] = 2.25
        for k, lift in enumerate([_f32(0.00001), one_ulp(0.00001, 0), one_ulp(0.00001, 1)]):      # 1e-5 -/+ ulp above the (flat) interpolated depth
            x, y = 60, 4 + 14 * k
            centre(x, y)
            n = neighbour(x, y, n_taps)
            if n and n[2]:
                position[n[2][0]][3] = _f32(2.0) + _f32(lift)
        for x, y in ((66, 3), (64, 10), (1, 1), (68, 43), (0, 44), (69, 0)):     # next to the background block; the image's corners (jittered texels outside)
            centre(x, y)
    elif name == "records":
        flat_all()
        counts = [0x0000, 0x0001, f16_bits(np.nextafter(np.float16(eps), np.float16(0)).astype(np.float32)), f16_bits(eps),
                  f16_bits(np.nextafter(np.float16(eps), np.float16(1)).astype(np.float32)), f16_bits(4.0), f16_bits(5.0), H_MAX, H_INF, H_NAN]
        for k, bits in enumerate(counts):                       # at a neighbour (tap 2), and at the centre itself one row below
            x, y = 4 + 7 * k, 3
            centre(x, y)
            n = neighbour(x, y, 2)
            if n:
                cur.count[n[0]] = bits
            # ... over a zero history record (the uv far outside) and with every tap refused (the normal turned away): the merged count
            # stays the pixel's own - below 1 for five of them, where the variance is NOT divided by the count
            cur.count[at(4 + 7 * k, 9)] = bits
            cur.lifetime[at(4 + 7 * k, 9)] = 0
            cur.visible_normal[at(4 + 7 * k, 9)] = (0, 0, -127)
            velocity[under(4 + 7 * k, 9)][:2] = 5.0
        # merged counts against max_spatial_reuse_count: a centre of count c over a zero history record whose taps all carry count 0 but
        # one: c + n == max, max + 1, max - 1
        for k, extra in enumerate((0, 1, -1)):
            x, y = 8 + 20 * k, 16
            fx, fy = fit(x, y)
            centre(x, y)
            if inside(fx, fy):
                for i in range(1, n_taps + 1):
                    n = neighbour(x, y, i)
                    if n:
                        cur.count[n[0]] = 0
                half_max = max_count // 2
                cur.count[fy, fx] = f16_bits(float(half_max))
                cur.lifetime[fy, fx] = 0                         # the history is asked for under every limit ...
                velocity[under(x, y)][:2] = 5.0                 # ... and previous_uv lies far outside: a zero record
                n = neighbour(x, y, 2)
                if n:
                    cur.count[n[0]] = f16_bits(float(max_count - half_max + extra))
        for k, bits in enumerate([0, H_MAX, H_INF, H_NAN]):     # w / w_sum / w2_sum at a neighbour and at the centre
            for j, field in enumerate(("w", "w_sum", "w2_sum")):
                x, y = 3 + 9 * k + 3 * j, 22
                centre(x, y)
                getattr(cur, field)[at(x, y)] = bits
                n = neighbour(x, y, 1)
                if n:
                    getattr(cur, field)[n[0]] = bits
        for k, bits in enumerate([0, H_NZERO, H_NAN, H_MAX]):   # radiance: total_lum > 0 false, NaN, the f16 maximum
            x, y = 40 + 7 * k, 22
            centre(x, y)
            cur.radiance[at(x, y)][:3] = bits
            hist.zero(at(x, y))
            n = neighbour(x, y, 1)
            if n:
                cur.radiance[n[0]][1] = bits
        # neighbour normals around dot = 0.866 against a centre normal (0, 0, 1): (sin a, 0, cos a) quantised, the z byte one step either way
        for k, nz in enumerate((109, 110, 111)):                # 110 / 127 = 0.8661: the bytes (63, 0, nz) normalise to a dot of 0.8679, 0.8678 ..
            x, y = 5 + 9 * k, 28
            centre(x, y)
            n = neighbour(x, y, 2)
            if n:
                cur.visible_normal[n[0]] = (64 + k - 1, 0, 110)
        for k, nrm in enumerate([(0, 0, 0), (0, 0, -127), (127, 0, 0), (60, 0, 112)]):      # zero (normalize(0)), anti-parallel, perpendicular, 28 degrees (a dot of 0.88: between 0.866 and 0.9)
            x, y = 34 + 7 * k, 28
            centre(x, y)
            n = neighbour(x, y, 2)
            if n:
                cur.visible_normal[n[0]] = nrm
            cur.visible_normal[at(34 + 7 * k, 31)] = nrm        # and at a centre
        # the neighbour's sample against the centre's visible position: on it (a zero-length direction), in the surface plane
        # (dot exactly 0), just in front, just behind
        for k, off in enumerate([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.0, 1e-6), (0.5, 0.0, -1e-6)]):
            x, y = 4 + 10 * k, 34
            centre(x, y)
            n = neighbour(x, y, 2)
            if n and inside(*fit(x, y)):
                cur.sample_position[n[0]] = cur.visible_position[at(x, y)][:3] + _f32(off)
            cur.sample_position[at(4 + 10 * k, 37)] = cur.visible_position[at(4 + 10 * k, 37)][:3] + _f32(off)      # the centre's own sample
        # the Jacobian: flag on / off x sample normal edge-on / averted / facing x near / far sample
        combos = [(flag, sn, dist) for flag in (127, 0) for sn in ((127, 0, 0), (0, 0, 127), (0, 0, -127)) for dist in (0.01, 30.0)]
        for k, (flag, sn, dist) in enumerate(combos):
            x, y = 3 + 5 * k, 41
            centre(x, y)
            n = neighbour(x, y, 1)
            if n:
                cur.jacobian_flag[n[0]], cur.sample_normal[n[0]] = flag, sn
                cur.sample_position[n[0]] = cur.visible_position[n[0]][:3] + _f32([0.0, 0.0, dist])
        limit = int(max_lifetime)
        for k, life in enumerate([max(limit - 1, 0), limit, limit + 1, 0, 1, 2, 253, 254]):      # at the centre: history taken or refused, the byte saturating on re-pack
            cur.lifetime[at(50 + 2 * k, 9)] = life
        for k, (code, _) in enumerate(quarter_turn_randoms(frame_number, n_taps)):                    # the tap angles nearest the quarter turns
            x, y = 62, 14 + 8 * k
            cur.random[at(x, y)] = (code, 0, 0, 0)
    elif name == "history":
        # previous_uv = jittered uv - velocity: the velocity is the pixel's own jittered uv minus the target, in f32
        targets = [(0.0, 0), (1.0, -1), (1.0, 0), (-0.25, 0), (np.nan, 0), (np.inf, 0), (-np.inf, 0), (1e9, 0), (0.5, 0), (0.25, 0)]
        sgn = _f32(-0.25) if frame_number % 2 == 0 else _f32(0.25)
        jr = _f32(_f32(p.frame.upscale_ratio) - _f32(1.0))
        for k, (target, nudge) in enumerate(targets):
            for axis in (0, 1):
                x, y = 3 + 6 * k, 4 + 12 * axis
                fx, fy = fit(x, y)
                if not inside(fx, fy):
                    continue
                size, coord, dsize = (rw, fx, dw) if axis == 0 else (rh, fy, dh)
                ju = _f32(_f32(_f32(coord + 0.5) / _f32(size)) + _f32(_f32(sgn * _f32(_f32(1.0) / _f32(dsize))) * jr))
                if np.isfinite(target):
                    vel = _f32(ju - _f32(target))
                    if nudge:                                    # one ulp under the target, as the shader forms it
                        while not _f32(ju - vel) < _f32(target):
                            vel = np.nextafter(vel, _f32(np.inf))
                        assert _f32(ju - vel) < _f32(target)
                else:
                    vel = _f32(-target) if not np.isnan(target) else _f32(np.nan)
                velocity[under(x, y)][axis] = vel
                cur.lifetime[at(x, y)] = 0                      # the history is asked for under every lifetime limit
        hist.zero((slice(0, rh // 3), slice(0, rw // 2)))      # a zero history record under a passing uv; the rest passes
    elif name == "background":
        # against the 8 x 8 wave tile and the 16 x 16 workgroup: columns 0..15 all background (one workgroup column), tiles 16..31 x
        # 0..15 geometry, then all-background tiles with ONE geometry pixel in each corner lane, and a NaN depth as a tile's only
        # non-background lane
        bg = np.zeros((rh + 1, rw + 1), bool)
        bg[:, :min(16, rw)] = True
        bg[16:32, 32:48] = True                                 # a background workgroup in the middle, geometry around it
        for tile_x, tile_y, (lx, ly) in ((4, 0, (0, 0)), (5, 0, (7, 0)), (4, 1, (0, 7)), (5, 1, (7, 7)), (6, 4, (3, 3))):
            bg[8 * tile_y:8 * tile_y + 8, 8 * tile_x:8 * tile_x + 8] = True
            if 8 * tile_y + ly < rh and 8 * tile_x + lx < rw:
                bg[8 * tile_y + ly, 8 * tile_x + lx] = False
                placed[8 * tile_y + ly, 8 * tile_x + lx] = True
        for y in range(rh):
            for x in range(rw):
                if bg[y, x]:
                    position[under(x, y, fitted=True)][3] = 0.0
        if rw > 8 * 6 + 3 and rh > 8 * 4 + 3:
            position[under(8 * 6 + 3, 8 * 4 + 3, fitted=True)][3] = np.nan
        background[...] = False
        cur.count[:, :min(8, rw)] = f16_bits(3.0)               # one tile column holds ONE record everywhere (the tile records' uniform case)
        for field in vars(cur):
            getattr(cur, field)[:, :min(8, rw)] = getattr(cur, field)[0, 0]
    position[background, 3] = 0.0
    if name == "terraces":      # (placed: the render pixels of the background block)
        for y in range(rh):
            for x in range(rw):
                if background[under(x, y, fitted=True)]:
                    placed[y, x] = True
    position, instance, velocity = position[:dh, :dw], instance[:dh, :dw], velocity[:dh, :dw]
    cur, hist, placed = cur.crop(rh, rw), hist.crop(rh, rw), placed[:rh, :rw]
    if name == "random":
        def some(shape, rate):
            return rng.random(shape) < rate

        for d in (0.0, np.nan, np.inf, -1.0, 1e-40, 2.25, 1.8):
            position[some((dh, dw), 0.01), 3] = d
        for r in (cur, hist):
            for bits in (0, 1, H_MAX, H_INF, H_NAN, f16_bits(4.0), f16_bits(5.0), f16_bits(float(max_count))):
                r.count[some((rh, rw), 0.01)] = bits
            for field in (r.w, r.w_sum, r.w2_sum):
                for bits in (0, H_MAX, H_INF, H_NAN):
                    field[some((rh, rw), 0.005)] = bits
            for bits in (0, H_NZERO, H_NAN, H_MAX):
                r.radiance[some((rh, rw, 4), 0.005)] = bits
            r.visible_normal[some((rh, rw), 0.01)] = 0
            r.visible_normal[some((rh, rw), 0.01)] = (0, 0, -127)
            r.lifetime[some((rh, rw), 0.03)] = 254
            r.lifetime[some((rh, rw), 0.03)] = 7
            m = some((rh, rw), 0.02)
            r.sample_position[m] = r.visible_position[m][:, :3]
        for v in (np.nan, np.inf, -np.inf, 1e9, -3.0, 0.5):
            velocity[some((dh, dw), 0.005), int(rng.integers(2))] = v
    p.current, p.previous_spatial, p.placed = cur, hist, placed
    sentinel_records = np.full((dh, dw, 16), SENTINEL_U32, np.uint32)

    def records_buffer(r):
        out = sentinel_records.copy()
        out.reshape(-1, 16)[:rw * rh] = pack_records(r).reshape(-1, 16)
        return out

    p.buffers = {F.BUF_POSITION: position, F.BUF_INSTANCE_MATERIAL: instance, F.BUF_VELOCITY_UV: velocity,
                 p.slots["current"]: records_buffer(cur), p.slots["previous_spatial"]: records_buffer(hist),
                 p.slots["spatial"]: sentinel_records.copy(), p.slots["previous"]: sentinel_records.copy(),
                 F.BUF_VARIANCE0 + channel: np.full((rh, rw, 1), SENTINEL_F32, np.float32),
                 F.BUF_RENDER0 + channel: np.full((rh, rw, 4), SENTINEL_F16, np.uint16)}
    p.buffers = {buf: np.ascontiguousarray(a) for buf, a in p.buffers.items()}
    return p


def install_spatial(engine, planes, resize=True):
    """hk_resize (if the size changed), hk_frame_begin with the planes' frame uniform, then every plane, record buffer and sentinel."""
    size = planes.window_size + (planes.ratio,)
    if resize and getattr(engine, "_post_planes_size", None) != size:
        engine.resize(*size)
        engine._post_planes_size = size
    camera = hk.cornell_camera(*planes.window_size)
    engine.frame_begin(planes.frame, camera.view_uniform(), camera.previous_view_uniform(None), hk.lights_uniform())
    for buf, array in planes.buffers.items():
        engine.write(buf, array)


# ------------------------------------------------------------------------------------------------------------------------------
# The three temporal light passes - direct_lit (sun, channel 0), direct_emissive (channel 1), indirect_lit_ambient (channel 2) - on a
# host-written G-buffer and a host-built `previous` reservoir buffer (light.wgsl:917-952, 1040-1240, 1452-1497).
#
# Sets (each places its specials deterministically; a small image gets the ones that fall inside it):
#   benign      every operand clear of every threshold: zero velocity, a history record that matches its pixel, counts 1 .. 20, radiance
#               0.05 .. 3, samples in the upper hemisphere - six in seven towards the sun, inside its cone.
#   edge        previous_uv in x, in y and in both, on the first, middle and last row and column: exactly 0, one ulp under 1, exactly 1,
#               one ulp over 1, negative, NaN, +-Inf, 1e9 - the velocity formed in f32 and the value it yields asserted (a -0 cannot be
#               formed: the difference of two equal finite operands is +0, so the planes place +0 there).  A uv.y of exactly 1, or a uv.x
#               of exactly 1 on the last row, forms a slot one row PAST the buffer: the store every scatter form must discard.  A uv.x of
#               exactly 1 on another row wraps to column 0 of the next row, in range, and is kept.  History records that pass and that
#               fail by depth, by normal and by instance alone.
#   thresholds  history depth either side of 1.05 * (1 + 0.5 * random.x) by one ulp, both directions of the ratio, at the pixels whose random.x
#               (the noise tile's: replayed, not chosen) is lowest, highest and nearest one half; current depth 0, epsilon -/+ ulp, NaN,
#               Inf, negative, denormal; history normals one snorm8 step either side of a dot of 0.9, zero and anti-parallel; instance ids
#               equal, off by one, NaN; counts 3, 4 and 4 -/+ one f16 ulp; counts that reach max_temporal_reuse_count exactly, pass it by
#               one, stay under it; history luminance - a grey f16 radiance under a validation ray that finds the sun - on adjacent f16
#               levels either side of a ratio of 1.25, of 0.8 and of the 0.0001 floor (`luminance_level`), and far above and below.
#   records     w / w_sum / w2_sum / radiance of 0, -0, 65504, Inf, NaN; lifetime bytes 0, 126, 127, 254; the history sample ON the visible
#               position (normalize(0)); samples below the surface.
#   scatter     a block of pixels whose history all reprojects onto ONE slot; a slot owned by a background pixel, and by a geometry pixel
#               that stores to itself; targets in another wave tile, another workgroup and far rows; chains a -> b -> c.  Run with the
#               validate intervals at 1 so that the second store (light.wgsl:1199-1202) happens on both parities.
#   background  as in the spatial planes: all-background tiles, one geometry pixel in a corner lane, a NaN depth as a tile's only geometry lane.
#   random      dense seeded noise with a few percent of each special.
TEMPORAL_SETS = ("benign", "edge", "thresholds", "records", "scatter", "background", "random")
TEMPORAL_PASSES = (F.PASS_DIRECT_LIT, F.PASS_DIRECT_EMISSIVE, F.PASS_INDIRECT)
TEMPORAL_SUN = dict(color=(1.0, 0.95, 0.9), illuminance=20000.0, direction_to_light=(0.3, 0.5, 0.8))
SURFACE_Z, GEOMETRY_Z, TANGENT_MARGIN = 2.0, -50.0, 1.0
EDGE_UVS = ("zero", "under_one", "one", "over_one", "negative", "nan", "inf", "ninf", "huge", "half")


def temporal_scene(kind):
    """`open`: the six material triangles of spatial_scene, far BELOW every surface point (make_temporal_planes asserts it): a ray that
    leaves the upper hemisphere of a visible normal hits nothing; no emitter.  `roofed`: the same, plus one large emissive quad above the
    surface points and one opaque occluder between it and the half x < 0 of them."""
    assert kind in ("open", "roofed")
    b = hk.SceneBuilder()
    mesh = b.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1]] * 3, [[0, 0], [1, 0], [0, 1]])
    for k, (colour, metallic, roughness) in enumerate(SPATIAL_MATERIALS):
        m = b.add_material(hk.standard_material(colour + (1.0,), perceptual_roughness=roughness, metallic=metallic, reflectance=0.3 + 0.1 * k))
        t = np.eye(4, dtype=np.float32)
        t[3, 0], t[3, 2] = 3.0 * k, GEOMETRY_Z
        b.add_instance(mesh, m, t)
    if kind == "roofed":
        quad = b.add_mesh([[-5, -5, 0], [5, -5, 0], [5, 5, 0], [-5, -5, 0], [5, 5, 0], [-5, 5, 0]], [[0, 0, -1]] * 6, [[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]])
        half = b.add_mesh([[-5, -5, 0], [0, -5, 0], [0, 5, 0], [-5, -5, 0], [0, 5, 0], [-5, 5, 0]], [[0, 0, -1]] * 6, [[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]])
        lamp = b.add_material(hk.standard_material((1.0, 1.0, 1.0, 1.0), emissive_linear=(4.0, 3.0, 2.0)))
        slab = b.add_material(hk.standard_material((0.5, 0.5, 0.5, 1.0)))
        for mesh_id, material, z in ((quad, lamp, 3.5), (half, slab, 3.0)):
            t = np.eye(4, dtype=np.float32)
            t[3, 1], t[3, 2] = 1.0, z
            b.add_instance(mesh_id, material, t)
    return b.finish()


def scene_triangle_vertices(scene):
    """world positions of every triangle vertex of a SceneData whose instances are pure translations (temporal_scene), float64"""
    v = np.array([[vt.position[0], vt.position[1], vt.position[2]] for vt in scene.vertices], np.float64)
    out = []
    for inst in scene.instances:
        m = np.array(list(inst.model), np.float64).reshape(4, 4)       # column-major: the translation is m[3, :3]
        assert np.allclose(m[:3, :3], np.eye(3))
        out.append(v + m[3, :3])
    return np.concatenate(out)


class TemporalPlanes:
    def __init__(self, name, seed, window_size, ratio, channel, frame_number, scene, settings):
        self.name, self.seed, self.window_size, self.ratio, self.channel, self.scene = name, seed, tuple(window_size), float(ratio), channel, scene
        self.settings = hk.HikariSettings(upscale=hk.Upscale.SmaaTu4x(ratio), **settings)
        self.frame = hk.frame_uniform(self.settings, frame_number)
        self.render_size = render_size_of(window_size, ratio)
        self.lights = hk.lights_uniform(TEMPORAL_SUN, ambient_brightness=0.3)
        cur = frame_number % 2
        prev = 1 - cur
        self.slots = {"previous": F.BUF_RESERVOIR0 + cur + T_SLOT[channel], "current": F.BUF_RESERVOIR0 + prev + T_SLOT[channel],
                      "previous_spatial": F.BUF_RESERVOIR0 + cur + S_SLOT[channel], "spatial": F.BUF_RESERVOIR0 + prev + S_SLOT[channel]}
        self.pass_id = TEMPORAL_PASSES[channel]
        self.buffers, self.placed, self.previous = {}, None, None

    @property
    def outputs(self):
        """what the pass writes, wholly or in part (the part it leaves alone keeps its sentinel)"""
        return {"current": self.slots["current"], "previous_spatial": self.slots["previous_spatial"], "spatial": self.slots["spatial"],
                "variance": F.BUF_VARIANCE0 + self.channel, "render": F.BUF_RENDER0 + self.channel}

    @property
    def untouched(self):
        """what it reads or must leave alone"""
        return {"previous": self.slots["previous"], "position": F.BUF_POSITION, "normal": F.BUF_NORMAL,
                "instance_material": F.BUF_INSTANCE_MATERIAL, "velocity_uv": F.BUF_VELOCITY_UV}


def temporal_jittered_uv(p, x, y):
    """jittered_deferred_uv(coords_to_uv(x, y), 0.25) in f32 (light.wgsl:1007-1011): (u, v)"""
    (dw, dh), (rw, rh) = p.window_size, p.render_size
    sgn = _f32(-0.25) if p.frame.number % 2 == 0 else _f32(0.25)
    ratio = _f32(_f32(p.frame.upscale_ratio) - _f32(1.0))
    u = _f32(_f32(_f32(x + 0.5) / _f32(rw)) + _f32(_f32(sgn * _f32(_f32(1.0) / _f32(dw))) * ratio))
    v = _f32(_f32(_f32(y + 0.5) / _f32(rh)) + _f32(_f32(sgn * _f32(_f32(1.0) / _f32(dh))) * ratio))
    return u, v


def _i32(v):
    """WGSL i32(f32) as the library and the oracle take it: truncation, saturating, NaN to 0"""
    v = float(v)
    if np.isnan(v):
        return 0
    return int(max(-2147483648.0, min(2147483520.0, np.trunc(v))))


def temporal_target(p, x, y, velocity):
    """What render pixel (x, y) makes of its velocity, in f32 as the shader does (light.wgsl:1081-1095): previous_uv, whether the LOAD
    reads history there (|uv - 0.5| < 0.5), whether the STORE condition holds (<= 0.5), and the slot index the store forms."""
    rw, rh = p.render_size
    with np.errstate(all="ignore"):
        ju, jv = temporal_jittered_uv(p, x, y)
        u, v = _f32(ju - _f32(velocity[0])), _f32(jv - _f32(velocity[1]))
        loads = bool(abs(_f32(u - _f32(0.5))) < _f32(0.5) and abs(_f32(v - _f32(0.5))) < _f32(0.5))
        stores = bool(abs(_f32(u - _f32(0.5))) <= _f32(0.5) and abs(_f32(v - _f32(0.5))) <= _f32(0.5))
        index = _i32(_f32(u * _f32(rw))) + rw * _i32(_f32(v * _f32(rh))) if stores else None
    return (u, v), loads, stores, index


def velocity_for(j, kind):
    """the f32 velocity component v for which f32(j - v) is the edge value `kind`, and that value - asserted; (None, None) where no f32
    velocity yields it from this j"""
    one = _f32(1.0)
    want = {"zero": _f32(0.0), "under_one": np.nextafter(one, _f32(0)), "one": one, "over_one": np.nextafter(one, _f32(2)), "negative": _f32(-0.25),
            "huge": _f32(1e9), "half": _f32(0.5)}.get(kind)
    with np.errstate(all="ignore"):
        if want is None:
            v = {"nan": _f32(np.nan), "inf": _f32(-np.inf), "ninf": _f32(np.inf)}[kind]
            got = _f32(j - v)
            assert np.isnan(got) if kind == "nan" else (np.isinf(got) and (got > 0) == (kind == "inf"))
            return v, got
        v = _f32(j - want)
        for _ in range(64):
            got = _f32(j - v)
            if got == want:
                break
            v = np.nextafter(v, _f32(-np.inf) if got < want else _f32(np.inf))
        if _f32(j - v) != want:        # (j an odd multiple of half the result's ulp: every difference is a tie, rounds to even, and skips odd targets)
            return None, None
        assert want < 0 or not np.signbit(_f32(j - v))
    return v, _f32(j - v)


def temporal_random_x(p, x, y):
    """s.random.x of render pixel (x, y): the noise tile's texel and fract(. + number * golden) in f32 (light.wgsl:1075-1080)"""
    n = int(p.frame.number)
    noise = hk.load_noise().reshape(16, 64, 64, 4)
    t = _f32(_f32(noise[n % 16, (y + n) % 64, (x + n) % 64, 0]) / _f32(255.0))
    s = _f32(t + _f32(_f32(n) * _f32(1.618033989)))
    return _f32(s - np.floor(s))


def f32_luminance(rgb):
    """luminance (utils.wgsl:63-65) in f32, the products summed in order"""
    r, g, b = (_f32(v) for v in rgb)
    return _f32(_f32(_f32(r * _f32(0.2126)) + _f32(g * _f32(0.7152))) + _f32(b * _f32(0.0722)))


def luminance_ratio_f32(p, grey_bits):
    """light.wgsl:1196: luminance(sun colour) / max(luminance(history radiance), 0.0001) in f32, the history radiance the f16 grey `grey_bits`"""
    g = np.uint16(grey_bits).view(np.float16).astype(np.float32)
    return _f32(f32_luminance(p.lights.directional_color[:3]) / max(f32_luminance((g, g, g)), _f32(0.0001)))


def luminance_level(p, target, side):
    """f16 bits of the grey history radiance that puts the validation's luminance ratio next to `target`: "1.25" / "0.8" - the last level
    whose ratio is above the threshold (`above`) or the first whose ratio is not (`below`), adjacent f16 values, the finest step the
    record's storage has; "floor" - the last level whose luminance is under the 0.0001 floor (`below`) or the first that is not.  Asserted."""
    levels = np.arange(1, 0x7C00, dtype=np.uint16)                                        # positive finite f16, ascending
    if target == "floor":
        lum = np.array([f32_luminance((g, g, g)) for g in levels.view(np.float16).astype(np.float32)[:0x0800]])
        first = int(np.argmax(lum >= _f32(0.0001)))
        assert lum[first] >= _f32(0.0001) > lum[first - 1]
        return levels[first - 1] if side == "below" else levels[first]
    thr = _f32(float(target))
    lo, hi = 0, len(levels) - 1                                                            # the ratio falls as the level rises
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if luminance_ratio_f32(p, levels[mid]) > thr else (lo, mid)
    assert luminance_ratio_f32(p, levels[lo]) > thr >= luminance_ratio_f32(p, levels[hi]) and hi == lo + 1
    return levels[lo] if side == "above" else levels[hi]


def make_temporal_planes(name, seed, render_size, ratio, channel, frame_number=2, scene="open", **settings):
    """One dispatch of temporal pass `channel` (0 sun, 1 emissive, 2 indirect) at `render_size`, the window being window_for(render_size,
    ratio); `settings` go to HikariSettings (indirect_bounces, validate intervals, max_temporal_reuse_count, temporal_reuse)."""
    assert name in TEMPORAL_SETS and channel in (0, 1, 2) and scene in ("open", "roofed")
    settings.setdefault("indirect_bounces", 1)
    settings.setdefault("emissive_spatial_reuse", True)             # previous_spatial of channels 0 and 1 has a reader: the library resolves their scatter by default
    if name == "scatter":
        settings.setdefault("direct_validate_interval", 1)
        settings.setdefault("emissive_validate_interval", 1)
    p = TemporalPlanes(name, seed, window_for(render_size, ratio), ratio, channel, frame_number, scene, settings)
    assert p.render_size == tuple(render_size)
    rng = np.random.default_rng([seed, 300 + TEMPORAL_SETS.index(name), channel])
    (dw, dh), (rw, rh) = p.window_size, p.render_size
    inside = lambda x, y: 0 <= x < rw and 0 <= y < rh
    placed = np.zeros((rh, rw), bool)
    p.branches, p.where = {}, {}                                     # what the set placed, by purpose: counts a test asserts to be non-zero, and (thresholds) where

    def note(key, n=1):
        p.branches[key] = p.branches.get(key, 0) + n

    def texel(x, y):
        """G-buffer [row, column] under render pixel (x, y), or None where the jittered texel lies outside"""
        tx, ty = spatial_texel(p, x, y)
        return (ty, tx) if 0 <= tx < dw and 0 <= ty < dh else None

    # ---- the G-buffer: a wall facing the camera of cornell_camera, every texel's normal in the upper hemisphere of +z
    gx, gy = np.meshgrid(np.arange(dw), np.arange(dh))
    depth = np.full((dh, dw), 2.0, np.float32) if name != "random" else (2.0 + 0.05 * rng.random((dh, dw))).astype(np.float32)
    position = np.zeros((dh, dw, 4), np.float32)
    position[..., 0], position[..., 1], position[..., 2], position[..., 3] = 0.02 * (gx - dw / 2), 1.0 + 0.02 * (dh / 2 - gy), SURFACE_Z, depth
    which = (gx // 11 + gy // 6) % 3
    normal3 = SPATIAL_NORMALS[which]
    instance = np.zeros((dh, dw, 2), np.float32)
    instance[..., 0] = (gx // 9 + gy // 7) % len(SPATIAL_MATERIALS)
    instance[..., 1] = instance[..., 0]
    velocity = np.zeros((dh, dw, 4), np.float32)
    velocity[..., 2:] = rng.random((dh, dw, 2))

    # ---- `previous`: per render pixel the record of the SAME surface point (zero velocity: previous_uv stays in the pixel)
    tex = np.array([[texel(x, y) or (0, 0) for x in range(rw)] for y in range(rh)])
    has_texel = np.array([[texel(x, y) is not None for x in range(rw)] for y in range(rh)])
    ty_, tx_ = tex[..., 0], tex[..., 1]
    hist = Records(rh, rw)
    shape = (rh, rw)
    hist.count[...] = f16_bits(rng.integers(1, 21, shape))
    hist.w[...] = f16_bits(0.1 + 1.9 * rng.random(shape))
    hist.w_sum[...] = f16_bits(0.5 + 9.5 * rng.random(shape))
    hist.w2_sum[...] = f16_bits(0.5 + 49.5 * rng.random(shape))
    hist.radiance[..., :3] = f16_bits(0.05 + 2.95 * rng.random(shape + (3,)))
    hist.radiance[..., 3] = H_ONE
    hist.random[...] = rng.integers(0, 65536, shape + (4,))
    hist.visible_position[...] = position[ty_, tx_]
    hist.visible_normal[...] = snorm8(normal3[ty_, tx_])
    hist.visible_instance[...] = instance[ty_, tx_, 0]
    lateral = 0.3 * (rng.random(shape + (3,)) - 0.5)
    hist.sample_position[...] = (hist.visible_position[..., :3] + 1.5 * normal3[ty_, tx_] + lateral).astype(np.float32)
    # six in seven history samples lie TOWARDS THE SUN, well inside its cone (solar_angle 0.046): a validation ray to them finds the sun,
    # and its radiance is known; the rest lie in the upper hemisphere outside the cone, where the validation ray finds nothing
    sun = np.asarray(TEMPORAL_SUN["direction_to_light"], np.float64) / np.linalg.norm(TEMPORAL_SUN["direction_to_light"])
    toward = sun + 0.01 * (rng.random(shape + (3,)) - 0.5)
    sunward = rng.random(shape) < 6.0 / 7.0
    hist.sample_position[sunward] = (hist.visible_position[..., :3] + 100.0 * toward / np.linalg.norm(toward, axis=-1, keepdims=True)).astype(np.float32)[sunward]
    hist.sample_normal[...] = snorm8(-normal3[ty_, tx_])
    hist.jacobian_flag[...] = np.where(rng.random(shape) < 0.5, 127, 0)
    hist.lifetime[...] = rng.integers(0, 11, shape)

    def put(x, y):
        placed[y, x] = True
        return y, x

    def aim(x, y, tx, ty):
        """the velocity that makes pixel (x, y) look at the centre of render pixel (tx, ty); asserted through temporal_target"""
        t = texel(x, y)
        if t is None:
            return False
        ju, jv = temporal_jittered_uv(p, x, y)
        velocity[t][0], velocity[t][1] = _f32(ju - _f32(_f32(tx + 0.5) / _f32(rw))), _f32(jv - _f32(_f32(ty + 0.5) / _f32(rh)))
        _, loads, stores, index = temporal_target(p, x, y, velocity[t][:2])
        assert loads and stores and index == tx + rw * ty, (x, y, tx, ty, index)
        put(x, y)
        return True

    def fail(y, x, reason):
        """make the history record at [y, x] fail check_previous_reservoir for ONE reason against a pixel that matches it otherwise"""
        if reason == "depth":
            hist.visible_position[y, x, 3] *= _f32(1.5)
        elif reason == "normal":
            hist.visible_normal[y, x] = snorm8(-normal3[ty_[y, x], tx_[y, x]])
        else:
            hist.visible_instance[y, x] += 1.0
        note("fails_" + reason)

    one_ulp = lambda v, towards: np.nextafter(_f32(v), _f32(towards))
    if name == "edge":
        cols, rows = sorted({0, rw // 2, rw - 1}), sorted({0, rh // 2, rh - 1})
        k = 0
        for y in range(rh):
            for x in range(rw):
                t = texel(x, y)
                if t is None or not (x in cols or y in rows):
                    if t is not None and (x + 2 * y) % 8 < 3:          # elsewhere: history that passes, or fails for one reason alone
                        fail(y, x, ("depth", "normal", "instance")[(x + 2 * y) % 8])
                    continue
                kind, axes = EDGE_UVS[k % len(EDGE_UVS)], ((0,), (1,), (0, 1))[(k // len(EDGE_UVS)) % 3]
                k += 7                                                  # (7 is coprime to 30: every value x axes combination comes round)
                if (x, y) == (rw - 1, rh - 1):
                    kind, axes = "one", (1,)                            # the slot one row past the buffer, in every shape
                elif (x, y) == (0, rh - 1) and rw > 1:
                    kind, axes = "one", (0,)                            # x exactly 1 on the last row: past the buffer as well
                elif (x, y) == (rw - 1, 0) and rh > 1:
                    kind, axes = "one", (0,)                            # x exactly 1 on another row: column 0 of the next row, kept
                j = temporal_jittered_uv(p, x, y)
                while any(velocity_for(j[a], kind)[0] is None for a in axes):       # (the next value that this pixel's uv can reach)
                    kind = EDGE_UVS[(EDGE_UVS.index(kind) + 1) % len(EDGE_UVS)]
                for a in axes:
                    velocity[t][a], _ = velocity_for(j[a], kind)
                put(x, y)
                (_u, _v), loads, stores, index = temporal_target(p, x, y, velocity[t][:2])
                note("uv_" + kind)
                if stores and not loads:
                    note("store_without_load")
                    note("store_discarded" if index >= rw * rh else "store_wrapped_in_range")
    elif name == "thresholds":
        k = 0
        cases = ([("depth", d, s) for d in (1, -1) for s in (1, -1)] + [("cur_depth", v, 0) for v in (0.0, np.nextafter(F32_EPSILON, _f32(0)), F32_EPSILON,
                 np.nextafter(F32_EPSILON, _f32(1)), np.nan, np.inf, -1.0, 1e-40)] + [("normal", z, 0) for z in (-2, -1, 0, 1, 2)] + [("normal_zero", 0, 0), ("normal_anti", 0, 0)] +
                 [("instance", v, 0) for v in (0.0, 1.0, np.nan)] + [("count", b, 0) for b in (f16_bits(3.0), f16_bits(4.0), f16_bits(4.0) - 1, f16_bits(4.0) + 1)] +
                 [("clamp", e, 0) for e in (-1, 0, 1, -10)] + [("luminance", v, 0) for v in ("1.25 above", "1.25 below", "0.8 above", "0.8 below", "floor above", "floor below", 0.0, 60000.0)])
        grid = [(x, y) for y in range(0, rh, 2) for x in range((y // 2) % 3, rw, 3) if texel(x, y) is not None]
        # the depth cases go where random.x - the noise tile's, not the set's to choose - is lowest, highest and nearest one half
        rx = {q: float(temporal_random_x(p, *q)) for q in grid}
        ranked = sorted(grid, key=lambda q: rx[q])
        middle = sorted(grid, key=lambda q: abs(rx[q] - 0.5))
        depth_cases, chosen = [c for c in cases if c[0] == "depth"], {}
        for group in (ranked, ranked[::-1], middle):
            for c in depth_cases:
                q = next((q for q in group if q not in chosen), None)
                if q is not None:
                    chosen[q] = c
        rest = [c for c in cases if c[0] != "depth"]
        for x, y in grid:
            t = texel(x, y)
            if (x, y) in chosen:
                what, a, b = chosen[(x, y)]
            else:
                what, a, b = rest[k % len(rest)]
                k += 1
            put(x, y)
            note(what)
            p.where.setdefault(what, []).append((x, y))
            d_cur = _f32(position[t][3])
            if what == "depth":                                     # history depth = current * (or /) the threshold, one ulp either side of it
                thr = _f32(_f32(1.05) * _f32(_f32(1.0) + _f32(_f32(0.5) * temporal_random_x(p, x, y))))
                d = _f32(d_cur * thr) if a > 0 else _f32(d_cur / thr)
                ratio = lambda d: (lambda q: _f32(_f32(1.0) / q) if q < 1 else q)(_f32(d / d_cur))
                # walk to the last depth whose ratio does not exceed the threshold, then (b > 0) one ulp beyond it
                away = _f32(np.inf) if a > 0 else _f32(0.0)
                for _ in range(64):
                    if ratio(d) > thr:
                        d = np.nextafter(d, _f32(d_cur))
                    elif not ratio(np.nextafter(d, away)) > thr:
                        d = np.nextafter(d, away)
                    else:
                        break
                assert not ratio(d) > thr and ratio(np.nextafter(d, away)) > thr
                hist.visible_position[y, x, 3] = np.nextafter(d, away) if b > 0 else d
            elif what == "cur_depth":
                position[t][3] = a
            elif what == "normal":                                  # the pixel's normal is +z; the history normal (s, 0, c) near a dot of 0.9
                normal3[t] = SPATIAL_NORMALS[0]
                hist.visible_normal[y, x] = (55 + a, 0, 114)        # normalised: 114 / hypot(55 + a, 114) = 0.9025 .. 0.8990 over a = -2 .. 2
            elif what == "normal_zero":
                hist.visible_normal[y, x] = 0
            elif what == "normal_anti":
                hist.visible_normal[y, x] = snorm8(-normal3[t])
            elif what == "instance":
                hist.visible_instance[y, x] = hist.visible_instance[y, x] + _f32(a)
            elif what == "count":
                hist.count[y, x] = a
            elif what == "clamp":
                hist.count[y, x] = f16_bits(float(max(0, p.settings.max_temporal_reuse_count + a)))
            elif what == "luminance":
                # validation with a count of 5: nothing is merged, the validation ray goes to the history sample - put inside the sun's
                # cone, so that on the open scene its radiance is the sun's colour - and the ratio is lum(sun) / max(lum(history), 1e-4).
                # The history radiance is f16: the grey level whose ratio is the last one above 1.25 (0.8), or the first one not above.
                hist.count[y, x] = f16_bits(5.0)
                hist.sample_position[y, x] = (hist.visible_position[y, x, :3] + 100.0 * sun).astype(np.float32)
                if isinstance(a, str):
                    target, side = a.split()
                    hist.radiance[y, x, :3] = luminance_level(p, target, side)
                else:
                    hist.radiance[y, x, :3] = f16_bits(a)
    elif name == "records":
        k = 0
        cases = ([(f, b) for f in ("w", "w_sum", "w2_sum", "radiance") for b in (0, H_NZERO, H_MAX, H_INF, H_NAN)] + [("lifetime", v) for v in (0, 126, 127, 254)] +
                 [("sample_on_surface", 0), ("sample_below", 0)])
        for y in range(rh):
            for x in range((y * 2) % 3, rw, 3):
                what, b = cases[k % len(cases)]
                k += 1
                put(x, y)
                note(what)
                if what == "radiance":
                    hist.radiance[y, x, :3] = b
                elif what == "lifetime":
                    hist.lifetime[y, x] = b
                elif what == "sample_on_surface":
                    hist.sample_position[y, x] = hist.visible_position[y, x, :3]
                elif what == "sample_below":
                    hist.sample_position[y, x] = hist.visible_position[y, x, :3] - _f32(1.5) * normal3[ty_[y, x], tx_[y, x]].astype(np.float32)
                else:
                    getattr(hist, what)[y, x] = b
                    if what == "w_sum":
                        hist.count[y, x] = f16_bits(2.0)
    elif name == "scatter":
        normal3[...] = SPATIAL_NORMALS[0]
        instance[...] = 2.0
        hist.visible_normal[...] = snorm8(SPATIAL_NORMALS[0])
        hist.visible_instance[...] = 2.0
        hist.count[...] = f16_bits(rng.integers(1, 4, shape))          # under 4: the new sample is merged, so every pixel's record differs
        hist.radiance[..., :3] = f16_bits(40.0 + 10.0 * rng.random(shape + (3,)))      # far from any validate radiance: the second store happens

        def owner_fails(tx, ty):
            if inside(tx, ty):
                fail(ty, tx, "depth")

        # many onto one slot, its history refused (first store) - and one onto a slot whose history passes (second store only)
        for target, block, refused in (((4, 2), [(x, y) for y in range(0, 4) for x in range(0, 8)], True),
                                       ((12, 9), [(x, y) for y in range(8, 12) for x in range(9, 16)], False)):
            if not inside(*target):
                continue
            if refused:
                owner_fails(*target)
            for x, y in block:
                if inside(x, y) and aim(x, y, *target):
                    note("contested")
        # the owner a background pixel / a geometry pixel that stores to itself (zero velocity, refused history)
        for target, sources in (((20, 3), [(22, 3), (19, 5)]), ((26, 3), [(24, 2), (30, 6)])):
            if not inside(*target) or texel(*target) is None:
                continue
            if target[0] == 20:
                position[texel(*target)][3] = 0.0
                note("owner_background")
            else:
                owner_fails(*target)
                note("owner_stores_to_itself")
            put(*target)
            for x, y in sources:
                if inside(x, y):
                    aim(x, y, *target)
        # another wave tile, another workgroup, far rows - in both directions (a lower and a higher index than the owner)
        for (x, y), target in (((33, 1), (44, 1)), ((44, 2), (33, 2)), ((2, 14), (50, 14)), ((66, 15), (3, 15)), ((5, 16), (60, 40)), ((61, 41), (6, 17)), ((3, 0), (3, 44)), ((8, 44), (8, 0))):
            if inside(x, y) and inside(*target):
                owner_fails(*target)
                if aim(x, y, *target):
                    note("far_target")
        # chains: a -> b -> c
        for a, b, c in (((40, 20), (42, 24), (45, 30)), ((30, 35), (28, 30), (25, 22)), ((1, 6), (2, 7), (3, 8))):
            if inside(*a) and inside(*b) and inside(*c):
                owner_fails(*b)
                owner_fails(*c)
                if aim(*a, *b) and aim(*b, *c):
                    note("chain")
    elif name == "background":
        bg = np.zeros((rh, rw), bool)
        bg[:, :min(16, rw)] = True
        bg[16:32, 32:48] = True
        for tile_x, tile_y, (lx, ly) in ((4, 0, (0, 0)), (5, 0, (7, 0)), (4, 1, (0, 7)), (5, 1, (7, 7)), (6, 4, (3, 3))):
            bg[8 * tile_y:8 * tile_y + 8, 8 * tile_x:8 * tile_x + 8] = True
            if 8 * tile_y + ly < rh and 8 * tile_x + lx < rw:
                bg[8 * tile_y + ly, 8 * tile_x + lx] = False
                placed[8 * tile_y + ly, 8 * tile_x + lx] = True
        for y in range(rh):
            for x in range(rw):
                if bg[y, x] and texel(x, y) is not None:
                    position[texel(x, y)][3] = 0.0
                    note("background")
        if rw > 8 * 6 + 3 and rh > 8 * 4 + 3 and texel(8 * 6 + 3, 8 * 4 + 3) is not None:
            position[texel(8 * 6 + 3, 8 * 4 + 3)][3] = np.nan
            note("nan_depth_lane")
    elif name == "random":
        some = lambda s, rate: rng.random(s) < rate
        for d in (0.0, np.nan, np.inf, -1.0, 1e-40, 2.25, 1.8):
            position[some((dh, dw), 0.01), 3] = d
        for bits in (0, 1, H_MAX, H_INF, H_NAN, f16_bits(3.0), f16_bits(4.0), f16_bits(5.0), f16_bits(float(p.settings.max_temporal_reuse_count))):
            hist.count[some(shape, 0.01)] = bits
        for field in (hist.w, hist.w_sum, hist.w2_sum):
            for bits in (0, H_NZERO, H_MAX, H_INF, H_NAN):
                field[some(shape, 0.005)] = bits
        for bits in (0, H_NZERO, H_NAN, H_MAX):
            hist.radiance[some(shape + (4,), 0.005)] = bits
        hist.visible_normal[some(shape, 0.01)] = 0
        hist.visible_normal[some(shape, 0.01)] = (0, 0, -127)
        hist.visible_instance[some(shape, 0.02)] += 1.0
        hist.visible_position[some(shape, 0.03), 3] *= _f32(1.2)
        hist.lifetime[some(shape, 0.03)] = 254
        m = some(shape, 0.02)
        hist.sample_position[m] = hist.visible_position[m][:, :3]
        hist.zero(some(shape, 0.05))
        for v in (np.nan, np.inf, -np.inf, 1e9, -3.0, 0.5):
            velocity[some((dh, dw), 0.005), int(rng.integers(2))] = v
        # a few percent look at another pixel's slot; one in a hundred at uv exactly 1 (the slot past the buffer, or the in-range wrap)
        for y in range(rh):
            for x in range(rw):
                t, r = texel(x, y), rng.random()
                if t is None or r > 0.06:
                    continue
                j = temporal_jittered_uv(p, x, y)
                if r < 0.01:
                    a = int(rng.integers(2))
                    velocity[t][a], _ = velocity_for(j[a], "one")
                else:
                    velocity[t][0] = _f32(j[0] - _f32(_f32(rng.integers(rw) + 0.5) / _f32(rw)))
                    velocity[t][1] = _f32(j[1] - _f32(_f32(rng.integers(rh) + 0.5) / _f32(rh)))

    # ---- the scene: out of reach where the set's name says so.  Every triangle vertex lies below the tangent plane of every
    # placed (or, for `benign`, every) surface point by TANGENT_MARGIN, in float64
    scene_data = temporal_scene(scene)
    if scene == "open":
        verts = scene_triangle_vertices(scene_data)
        pts, nrm = position[..., :3].reshape(-1, 3).astype(np.float64), normal3.reshape(-1, 3)
        below = ((verts[None, :, :] - pts[:, None, :]) * nrm[:, None, :]).sum(axis=2)
        assert below.max() < -TANGENT_MARGIN, below.max()
    p.scene_data = scene_data
    p.previous, p.placed = hist, placed
    sentinel_records = np.full((dh, dw, 16), SENTINEL_U32, np.uint32)
    previous = sentinel_records.copy()
    previous.reshape(-1, 16)[:rw * rh] = pack_records(hist).reshape(-1, 16)
    normal = pack_snorm8x4(np.concatenate([normal3, np.zeros((dh, dw, 1))], axis=2))[..., None]
    p.buffers = {F.BUF_POSITION: position, F.BUF_NORMAL: normal, F.BUF_INSTANCE_MATERIAL: instance, F.BUF_VELOCITY_UV: velocity,
                 p.slots["previous"]: previous, p.slots["current"]: sentinel_records.copy(), p.slots["previous_spatial"]: sentinel_records.copy(),
                 p.slots["spatial"]: sentinel_records.copy(),
                 F.BUF_VARIANCE0 + channel: np.full((rh, rw, 1), SENTINEL_F32, np.float32),
                 F.BUF_RENDER0 + channel: np.full((rh, rw, 4), SENTINEL_F16, np.uint16)}
    p.buffers = {buf: np.ascontiguousarray(a) for buf, a in p.buffers.items()}
    return p


def temporal_store_targets(p):
    """Per geometry pixel of the planes, in f32 as the shader forms them: the slot index where the store condition holds.  Returns
    (indices, counts, unloaded): `indices` [rh, rw] int64 with -1 where the condition fails or the pixel is background, `counts` a dict
    of outside / in_range / to_own_slot / to_other_slot / wrapped_in_range (stores without a load that stay inside) / discarded (>= rw *
    rh), `unloaded` [rh, rw] bool: the store condition holds and the load's does not - a zero record, always refused, so the pixel DOES store."""
    (dw, dh), (rw, rh) = p.window_size, p.render_size
    position, velocity = p.buffers[F.BUF_POSITION], p.buffers[F.BUF_VELOCITY_UV]
    out, unloaded = np.full((rh, rw), -1, np.int64), np.zeros((rh, rw), bool)
    counts = dict(background=0, outside=0, in_range=0, to_own_slot=0, to_other_slot=0, wrapped_in_range=0, discarded=0)
    for y in range(rh):
        for x in range(rw):
            tx, ty = spatial_texel(p, x, y)
            d = position[ty, tx, 3] if 0 <= tx < dw and 0 <= ty < dh else _f32(0.0)
            if d < F32_EPSILON:
                counts["background"] += 1
                continue
            vel = velocity[ty, tx, :2] if 0 <= tx < dw and 0 <= ty < dh else _f32([0.0, 0.0])
            _, loads, stores, index = temporal_target(p, x, y, vel)
            if not stores:
                counts["outside"] += 1
                continue
            out[y, x], unloaded[y, x] = index, not loads
            if index >= rw * rh or index < 0:
                counts["discarded"] += 1
                assert not loads
                continue
            counts["in_range"] += 1
            counts["to_own_slot" if index == x + rw * y else "to_other_slot"] += 1
            if not loads:
                counts["wrapped_in_range"] += 1
    return out, counts, unloaded


def install_temporal(engine, planes, resize=True):
    """hk_resize (if the size changed), hk_frame_begin with the planes' frame uniform and lights, then every plane, record buffer and
    sentinel.  The engine must hold temporal_scene(planes.scene)."""
    size = planes.window_size + (planes.ratio,)
    if resize and getattr(engine, "_post_planes_size", None) != size:
        engine.resize(*size)
        engine._post_planes_size = size
    camera = hk.cornell_camera(*planes.window_size)
    engine.frame_begin(planes.frame, camera.view_uniform(), camera.previous_view_uniform(None), planes.lights)
    for buf, array in planes.buffers.items():
        engine.write(buf, array)


def dump_temporal_planes(planes, path):
    """Everything one dispatch needs, as a flat file a stand-alone program can replay without Python (tests/native/
    temporal_oracle_main.cpp): a sequence of blobs, each a u64 byte count and the bytes - a header (window width, height, the ratio's
    f32 bits, the pass id, the number of buffers), the nine scene arrays in SceneData.FIELDS order, the noise tiles, HkFrame, HkView,
    HkPreviousView, HkLights, then per buffer its id (u32) and its contents."""
    import ctypes as C
    import struct

    camera = hk.cornell_camera(*planes.window_size)
    blobs = [struct.pack("<IIfII", planes.window_size[0], planes.window_size[1], planes.ratio, planes.pass_id, len(planes.buffers))]
    blobs += [bytes(memoryview(getattr(planes.scene_data, k))) for k in hk.SceneData.FIELDS]
    blobs += [hk.load_noise().tobytes()]
    blobs += [bytes(memoryview(s)) if isinstance(s, (C.Structure, C.Array)) else bytes(s)
              for s in (planes.frame, camera.view_uniform(), camera.previous_view_uniform(None), planes.lights)]
    for buf, array in planes.buffers.items():
        blobs += [struct.pack("<I", buf), array.tobytes()]
    with open(path, "wb") as f:
        for b in blobs:
            f.write(struct.pack("<Q", len(b)))
            f.write(b)
