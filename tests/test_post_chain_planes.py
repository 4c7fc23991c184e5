"""The oracle's demodulation, a-trous levels and tone mapping against a float64 restatement of denoise.wgsl / tone_mapping.wgsl on
the adversarial planes of tests/post_planes.py - one dispatch at a time, each level fed what the oracle wrote for the previous one.

The restatement below is written from the shaders' text alone; it uses none of the numeric contract's functions (the kernels and the
oracle share those, so a mistake in one of them cancels in a GPU-vs-oracle comparison).  The shader's order of operations decides
every discrete choice; the reference returns its output, one mask per decision, a `margin` mask (its own decision lies within
rounding distance of a threshold) and a `dont_care` mask (the value hangs on something WGSL leaves open: max / clamp of a NaN,
normalize of a zero vector, pow of a negative or NaN base, sqrt of a negative number).  Texels in neither mask must agree: NaN-ness,
the sign of an infinity and exact zeros exactly, everything else within BOUND_ULPS f16 ulps (BOUND_VARIANCE for the f32
`internal_variance`, relative, in units of 2^-24).  The bounds are twice the worst deviation measured over all plane sets, rounded
up to a whole ulp: DESIGN.md section 2, "The post chain against float64".

At most 2 % of the geometry texels of any one dispatch may be left out (measured: at most 1.9 %), and no texel a set
placed deliberately may be left out because of a margin.  That share is asserted on SHAPES, images of 585 texels and more.  On
EDGE_SHAPES (1 wide or 1 high: every tap of one direction is outside the image) the same deviations, special values and placed
texels are held, and the cap is 2 % rounded up to a whole texel over everything but the firefly margin: there a texel has two taps,
`ff_var` is ((a - b) / 2)^2, and the test `lum > mean + 3 sigma` hangs on rounding at every local maximum of the smoothed line whose
two neighbours agree to 0.2 % - how many there are follows from the filter, not from a share of the image.  For the three sets whose
specials are laid out for one level's step (WRITTEN_LEVELS) every level is also run straight on the demodulated plane, and the
branch counts are asserted per level."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F

# twice the measured worst deviations (0.500, 0.503, 0.500 ulp; 3.45 x 2^-24), rounded up: DESIGN.md section 2
BOUND_ULPS = {"demodulation": 1, "denoise": 2, "tone_mapping": 1}
BOUND_VARIANCE = 7          # relative, in units of 2^-24: nine products summed in f32
EXCLUDED_CAP = 0.02

F32_MAX = float(np.float32(3.402823466e38))
F32_EPSILON = float(np.float32(1.1920929e-7))
LUMA = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], dtype=np.float64)
OFFSETS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]           # the order of the calls in denoise()
VARIANCE_OFFSETS = [(ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1)]                   # ... and in demodulation()
SHAPES = [(130, 17), (65, 9), (63, 17), (64, 17), (130, 9)]
EDGE_SHAPES = [(1, 1), (1, 9), (1, 17), (64, 1), (130, 1)]      # every tap of one direction outside the image


def half(u16):
    return u16.view(np.float16).astype(np.float64)


class Geometry:
    """what the shaders read from the frame uniform and the G-buffer, in float64"""

    def __init__(self, planes, transpose_kernel=False):
        self.dw, self.dh = planes.window_size
        self.rw, self.rh = planes.render_size
        f = planes.frame
        k = np.array([[f.kernel[c][r] for r in range(3)] for c in range(3)], dtype=np.float64)
        self.kernel = k.T.copy() if transpose_kernel else k                      # kernel[a][b] = frame.kernel[a][b]
        self.jitter = (-0.5 if f.number % 2 == 0 else 0.5) * (float(np.float32(f.upscale_ratio)) - 1.0)
        self.clear = np.array([f.clear_color[i] for i in range(4)], dtype=np.float64)
        self.indirect = f.indirect_bounces != 0
        self.depth = planes["position"][..., 3].astype(np.float64)
        self.gradient = planes["depth_gradient"].astype(np.float64)
        self.instance = planes["instance_material"][..., 0].astype(np.float64)
        self.albedo = half(planes["albedo"])
        n = np.maximum(planes["normal"].view(np.int8).reshape(self.dh, self.dw, 4)[..., :3].astype(np.float64) / 127.0, -1.0)
        with np.errstate(all="ignore"):
            self.normal = n / np.sqrt((n * n).sum(axis=2, keepdims=True))         # normalize(0): NaN here, open in WGSL
        self.y, self.x = np.meshgrid(np.arange(self.rh), np.arange(self.rw), indexing="ij")

    def deferred(self, x, y):
        """nearest G-buffer texel under jittered_deferred_uv(coords_to_uv(x, y)), and whether it is within rounding of another"""
        fx = (x + 0.5) / self.rw * self.dw + self.jitter
        fy = (y + 0.5) / self.rh * self.dh + self.jitter
        close = (np.abs(fx - np.rint(fx)) < 1e-4) | (np.abs(fy - np.rint(fy)) < 1e-4)
        tx = np.clip(np.floor(fx), 0, self.dw - 1).astype(np.int64)
        ty = np.clip(np.floor(fy), 0, self.dh - 1).astype(np.int64)
        return tx, ty, close

    def inside(self, x, y):
        u, v = (x + 0.5) / self.rw, (y + 0.5) / self.rh
        return ~((u < 0.0) | (v < 0.0) | (u > 1.0) | (v > 1.0))


def rejected(irr, nan_skip=True):
    above = (irr > F32_MAX).any(axis=-1)
    return (np.isnan(irr).any(axis=-1) | above) if nan_skip else above


def ref_demodulation(g, render, variance):
    with np.errstate(all="ignore"):
        tx, ty, close = g.deferred(g.x, g.y)
        albedo = g.albedo[ty, tx, :3]
        irr = half(render)[..., :3]
        out = np.concatenate([np.where(albedo < 0.01, 0.0, irr / albedo), np.ones((g.rh, g.rw, 1))], axis=2)
        total, dont_care = np.zeros((g.rh, g.rw)), np.zeros((g.rh, g.rw), bool)
        skipped = 0
        var = variance[..., 0].astype(np.float64)
        for ox, oy in VARIANCE_OFFSETS:
            sx, sy = g.x + ox, g.y + oy
            ins = g.inside(sx, sy)
            v = var[np.clip(sy, 0, g.rh - 1), np.clip(sx, 0, g.rw - 1)]
            skip = v > F32_MAX
            take = ins & ~skip
            dont_care |= take & np.isnan(v)                                       # max(NaN, 0.0)
            total += np.where(take, g.kernel[oy + 1][ox + 1] * np.maximum(v, 0.0), 0.0)
            skipped += int((ins & skip).sum())
    return {"out": out, "variance": total, "margin": close, "dont_care": np.zeros_like(close), "variance_dont_care": dont_care,
            "counts": {"variance_skips": skipped, "albedo_zeroed": int((albedo < 0.01).sum())}}


def ref_denoise(g, level, firefly, inp, ivar, mistake=None):
    step = 8 >> level
    with np.errstate(all="ignore"):
        tx, ty, margin = g.deferred(g.x, g.y)
        depth, gradient, normal, instance = g.depth[ty, tx], g.gradient[ty, tx], g.normal[ty, tx], g.instance[ty, tx]
        background = depth < F32_EPSILON
        tex = half(inp)[..., :3]
        var = ivar[..., 0].astype(np.float64)
        rej_c = rejected(tex, mistake != "no_nan_skip")
        kc = g.kernel[1][1]
        irr = np.where(rej_c[..., None], 0.0, tex)
        sum_irr, sum_w = irr * np.where(rej_c, 0.0, kc)[..., None], np.where(rej_c, 0.0, kc)
        lum = irr @ LUMA
        denominator = 4.0 * np.power(var, 0.25) + 0.001
        dont_care = np.zeros((g.rh, g.rw), bool)
        m1, m2, count = np.zeros((g.rh, g.rw)), np.zeros((g.rh, g.rw)), np.zeros((g.rh, g.rw))
        taps_inside, taps_rejected = np.zeros((g.rh, g.rw), int), np.zeros((g.rh, g.rw), int)
        for ox, oy in OFFSETS:
            sx, sy = g.x + ox * step, g.y + oy * step
            ins = g.inside(sx, sy)
            t = tex[np.clip(sy, 0, g.rh - 1), np.clip(sx, 0, g.rw - 1)]
            rej = rejected(t, mistake != "no_nan_skip")
            take = ins & ~rej
            taps_inside += ins
            taps_rejected += ins & rej
            sxt, syt, close = g.deferred(sx, sy)
            margin |= take & close
            sl = t @ LUMA
            d = (normal * g.normal[syt, sxt]).sum(axis=2)
            w_normal = np.power(np.maximum(0.0, d), 16.0)
            w_depth = np.exp(-np.abs(depth - g.depth[syt, sxt]) / (np.abs(gradient[..., 0] * ox + gradient[..., 1] * oy) + 0.01))
            di = 1.0 - np.abs(instance - g.instance[syt, sxt])
            w_instance = np.maximum(0.0, di)
            w_luminance = np.exp(-np.abs(lum - sl) / denominator)
            product = w_normal * w_depth * w_instance * w_luminance
            open_ = np.isnan(d) | np.isnan(di) | np.isnan(product) | (var < 0.0) | np.isnan(var)      # max / clamp / pow of what WGSL leaves open
            dont_care |= take & open_
            ka, kb = (ox + 1, oy + 1) if mistake == "transposed_kernel" else (oy + 1, ox + 1)
            w = np.clip(product, 0.0, 1.0) * g.kernel[ka][kb]
            margin |= take & np.isinf(t).any(axis=-1) & (product > 0.0) & (product < 1e-30)     # (-Inf * 0 is NaN, -Inf * tiny is not: f32 underflows earlier)
            sum_irr = sum_irr + np.where(take[..., None], t * w[..., None], 0.0)
            sum_w = sum_w + np.where(take, w, 0.0)
            m1, m2, count = m1 + np.where(take, sl, 0.0), m2 + np.where(take, sl * sl, 0.0), count + take
        fallback = sum_w < 0.0001
        margin |= np.abs(sum_w - 0.0001) < 1e-8
        out = np.where(fallback[..., None], 0.0, sum_irr / sum_w[..., None])
        fired = firefly_margin = np.zeros((g.rh, g.rw), bool)
        if firefly or mistake == "firefly_on_channel_0":
            mean = m1 / count
            ff_var = m2 / count - mean * mean
            tol = 1e-6 * np.abs(m2 / count)                                        # what f32 rounding can move ff_var by (none when every tap is 0)
            lo, hi = mean + 3.0 * np.sqrt(np.maximum(ff_var - tol, 0.0)), mean + 3.0 * np.sqrt(np.maximum(ff_var + tol, 0.0))
            nonnegative = (ff_var > tol) | (((tol == 0.0) | (count == 1)) & (ff_var == 0.0))      # (ff_var < 0 in f32: sqrt is NaN / open, the test false; one tap: 0 exactly)
            sure_true = nonnegative & (lum > hi + 1e-5 * np.abs(hi))
            sure_false = ~(lum > lo - 1e-5 * np.abs(lo))
            firefly_margin = ~(sure_true | sure_false) & ~(np.abs(mean / lum - 1.0) < 1e-5)      # (a factor of 1 +- 1e-5 either way: not a decision)
            margin |= firefly_margin
            fired = sure_true
            out = np.where(fired[..., None], (mean / lum)[..., None] * out, out)
        color = np.concatenate([out, np.ones((g.rh, g.rw, 1))], axis=2)
        if level == 3:
            color = color * g.albedo[ty, tx]
        overflow = np.isfinite(color).all(axis=2) & (np.abs(color) >= 65520.0).any(axis=2) & ~background
        color[background] = 0.0
        geometry = ~background
    return {"out": color, "margin": margin & geometry, "dont_care": dont_care & geometry, "geometry": geometry, "firefly_margin": firefly_margin & geometry,
            "counts": {"rejected_centres": int((rej_c & geometry).sum()), "rejected_taps": int(taps_rejected[geometry].sum()),
                       "all_taps_rejected": int(((taps_rejected == taps_inside) & (taps_inside > 0) & geometry).sum()),
                       "rejected_centre_and_all_taps": int(((taps_rejected == taps_inside) & (taps_inside > 0) & rej_c & geometry).sum()),
                       "ff_count_zero": int(((count == 0) & geometry).sum()) if firefly else 0,
                       "firefly_clamps": int((fired & geometry).sum()), "sum_w_fallbacks": int((fallback & geometry).sum()),
                       "f16_overflows": int(overflow.sum()) if level == 3 else 0, "background": int(background.sum())}}


def ref_tone_mapping(g, direct, emissive, indirect):
    with np.errstate(all="ignore"):
        color = half(direct) + half(emissive)
        color = color + (half(indirect) if g.indirect else 0.0)      # (no bounces: post_process.rs:949-954 binds an all-zero fallback texture)
        dont_care = np.isnan(color[..., :3]).any(axis=2)                           # max(NaN, 0.0039)
        rgb = np.maximum(color[..., :3], float(np.float32(0.0039)))
        l_old = rgb @ LUMA
        l_new = l_old / (1.0 + l_old)
        mapped = np.concatenate([rgb * (l_new / l_old)[..., None], color[..., 3:4]], axis=2)
        keep = color[..., 3] > 0.0
        out = np.where(keep[..., None], mapped, g.clear)
    return {"out": out, "margin": np.zeros_like(keep), "dont_care": dont_care & keep, "geometry": np.ones_like(keep),
            "counts": {"clear_colour_selects": int((~keep).sum()), "alpha_nan": int(np.isnan(color[..., 3]).sum())}}


def f16_ulp(v):
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)


def deviation_f16(want, got_bits, skip):
    """(worst deviation in f16 ulps, texels whose special values disagree) over the texels not in `skip`"""
    got = half(got_bits)
    with np.errstate(all="ignore"):
        near_overflow = np.abs(np.abs(want) - 65520.0) < 1.0
        skip = skip[..., None] | near_overflow
        nan, inf, zero = np.isnan(want), np.abs(want) >= 65520.0, want == 0.0
        special_bad = (nan != np.isnan(got)) | (inf & ~nan & (got != np.sign(want) * np.inf)) | (~inf & ~nan & np.isinf(got)) | (zero & (got != 0.0))
        ordinary = ~nan & ~inf & ~zero & ~skip & ~special_bad
        dev = np.where(ordinary, np.abs(got - want) / f16_ulp(want), 0.0)
    return float(dev.max(initial=0.0)), (special_bad & ~skip).any(axis=2)


def deviation_f32(want, got, skip):
    got = got[..., 0].astype(np.float64)
    with np.errstate(all="ignore"):
        bad = ((want == 0.0) != (got == 0.0)) | ~np.isfinite(got)
        dev = np.where(~skip & ~bad & (want != 0.0), np.abs(got - want) / np.maximum(np.abs(want) * 2.0 ** -24, 2.0 ** -149), 0.0)     # (f32 denormals: absolute)
    return float(dev.max(initial=0.0)), bad & ~skip


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import oracle_plugin

    p = oracle_plugin()
    p.set_scene(hk.load_cornell())
    return p.engine


def dispatches(e, planes, mistake=None, written_levels=False):
    """Run the post chain on the oracle dispatch by dispatch; per dispatch yield (kind, label, reference result, what the oracle wrote)."""
    PP.install(e, planes)
    g = Geometry(planes, transpose_kernel=False)
    for ch in range(planes.channels):
        e.pass_run(F.PASS_DEMODULATION, ch)
        r = ref_demodulation(g if mistake != "transposed_kernel" else Geometry(planes, True), planes.buffers[F.BUF_RENDER0 + ch], planes.buffers[F.BUF_VARIANCE0 + ch])
        yield "demodulation", f"demodulation ch{ch}", r, e.read(F.BUF_DENOISE_INTERNAL0), e.read(F.BUF_DENOISE_INTERNAL_VARIANCE)
        demodulated = e.read(F.BUF_DENOISE_INTERNAL0)
        for level in range(4):
            if written_levels:        # every level straight on the demodulated plane: the lit texel of `black` is a tap at this level's step
                e.write(F.BUF_DENOISE_INTERNAL0 + level, demodulated)
            inp, ivar = e.read(F.BUF_DENOISE_INTERNAL0 + level), e.read(F.BUF_DENOISE_INTERNAL_VARIANCE)
            e.pass_run(F.PASS_DENOISE_L0 + level, ch)
            r = ref_denoise(g, level, ch > 0, inp, ivar, mistake)
            if mistake:               # (what may be left out is decided by the shader as written, not by the planted mistake)
                right = ref_denoise(g, level, ch > 0, inp, ivar)
                r["margin"], r["dont_care"] = right["margin"], right["dont_care"]
            r["input"], r["level"], r["channel"] = inp, level, ch
            yield "denoise", f"denoise_l{level} ch{ch}", r, e.read(F.BUF_DENOISE_RENDER0 + ch if level == 3 else F.BUF_DENOISE_INTERNAL0 + level + 1), None
    for denoised in (1, 0):
        base = F.BUF_DENOISE_RENDER0 if denoised else F.BUF_RENDER0
        ins = [e.read(base + i) for i in range(3)]
        e.pass_run(F.PASS_TONE_MAPPING, denoised)
        yield "tone_mapping", f"tone_mapping({denoised})", ref_tone_mapping(g, *ins), e.read(F.BUF_TONE_MAPPED), None


def black_waves(r):
    """(waves of 64 x 1 whose geometry pixels are all black under their whole stencil, waves black but for one lane) - the two cases of
    the shortcut in k_denoise, counted on the level's input bits (+0 only; a tap outside the image counts as black)"""
    inp, step = r["input"], 8 >> r["level"]
    h, w = inp.shape[:2]
    lit = (inp[..., :3] != 0).any(axis=2)
    pad = np.zeros((h + 2 * step, w + 2 * step), bool)
    pad[step:step + h, step:step + w] = lit
    stencil = np.zeros((h, w), bool)
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            stencil |= pad[step + oy * step:step + oy * step + h, step + ox * step:step + ox * step + w]
    whole = one = 0
    for y in range(h):
        for x0 in range(0, w, 64):
            geo = r["geometry"][y, x0:x0 + 64]
            n = int((stencil[y, x0:x0 + 64] & geo).sum())
            whole, one = whole + (geo.any() and n == 0), one + (n == 1)
    return whole, one


def check(planes, records, placed, edge=False):
    """Compare every dispatch; returns {kind: worst deviation}, the worst excluded share and texel count, the branch counts summed and
    per level, and the problems."""
    worst, share, left_out, counts, by_level, problems = {}, 0.0, 0, {}, {}, []
    for kind, label, r, got, got_variance in records:
        skip = r["margin"] | r["dont_care"]
        dev, bad = deviation_f16(r["out"], got, skip)
        worst[kind] = max(worst.get(kind, 0.0), dev)
        if bad.any():
            ys, xs = np.nonzero(bad)
            problems.append(f"{label}: {int(bad.sum())} texels disagree on NaN / Inf / zero, first (x={xs[0]}, y={ys[0]}): {half(got)[ys[0], xs[0]]} vs {r['out'][ys[0], xs[0]]}")
        if dev > BOUND_ULPS[kind]:
            problems.append(f"{label}: {dev:.2f} ulp > {BOUND_ULPS[kind]}")
        if got_variance is not None:
            vdev, vbad = deviation_f32(r["variance"], got_variance, r["variance_dont_care"])
            worst["internal_variance"] = max(worst.get("internal_variance", 0.0), vdev)
            if vbad.any() or vdev > BOUND_VARIANCE:
                problems.append(f"{label}: internal_variance {vdev:.2f} x 2^-24, {int(vbad.sum())} special")
            skip = skip | r["variance_dont_care"]
        geometry = r.get("geometry", np.ones_like(skip))
        n = max(1, int(geometry.sum()))
        share, left_out = max(share, float((skip & geometry).sum()) / n), max(left_out, int((skip & geometry & ~r.get("firefly_margin", False)).sum()) - int(np.ceil(EXCLUDED_CAP * n)))
        placed_margin = r["margin"] & placed & ~(r.get("firefly_margin", False) if edge else False)      # (edge shapes: the module docstring)
        if placed_margin.any():
            problems.append(f"{label}: {int(placed_margin.sum())} deliberately placed texels lie within rounding of a threshold")
        for k, v in r["counts"].items():
            counts[k] = counts.get(k, 0) + v
            if kind == "denoise":
                by_level.setdefault(r["level"], {})[k] = by_level.setdefault(r["level"], {}).get(k, 0) + v
        if kind == "denoise":
            whole, one = black_waves(r)
            counts["black_waves"], counts["one_lane_waves"] = counts.get("black_waves", 0) + whole, counts.get("one_lane_waves", 0) + one
            lv = by_level.setdefault(r["level"], {})
            lv["black_waves"], lv["one_lane_waves"] = lv.get("black_waves", 0) + int(whole), lv.get("one_lane_waves", 0) + one
    return worst, share, left_out, counts, by_level, problems


_measured = {}


WRITTEN_LEVELS = ("nonfinite", "thresholds", "black")      # sets whose specials are laid out for one level's step: see dispatches()


@pytest.mark.parametrize("name", PP.SETS)
def test_oracle_agrees_with_float64(oracle, name):
    total, levels, problems, worst_share, shares, over = {}, {}, [], 0.0, {}, {}
    for shape in SHAPES + EDGE_SHAPES:
        for ratio, parity in ((1.0, 2), (1.5, 3), (1.5, 2)):
            planes = PP.make_planes(name, 7, PP.window_for(shape, ratio), ratio, 3, parity)
            for written in ((False, True) if name in WRITTEN_LEVELS else (False,)):
                worst, share, left_out, counts, by_level, bad = check(planes, dispatches(oracle, planes, written_levels=written), planes.placed, edge=shape in EDGE_SHAPES)
                problems += [f"{shape} x{ratio} f{parity}{' written' if written else ''}: {b}" for b in bad]
                for k, v in worst.items():
                    _measured[k] = max(_measured.get(k, 0.0), v)
                shares[shape] = max(shares.get(shape, 0.0), share)
                if shape in SHAPES:
                    worst_share = max(worst_share, share)
                elif left_out > 0:
                    over[(shape, ratio, parity, written)] = left_out
                if shape == SHAPES[0]:
                    for k, v in counts.items():
                        total[k] = total.get(k, 0) + v
                    if written or name not in WRITTEN_LEVELS:
                        for level, c in by_level.items():
                            for k, v in c.items():
                                levels.setdefault(level, {})[k] = levels.setdefault(level, {}).get(k, 0) + v
    print(name, "worst deviations so far", {k: round(v, 3) for k, v in _measured.items()}, "left-out share", {k: round(v, 4) for k, v in shares.items()}, "branches", total,
          "per level", levels)
    assert problems == []
    assert worst_share <= EXCLUDED_CAP, worst_share
    assert over == {}          # the edge shapes: see the module docstring
    # the branches the set is for really ran (counts over the 130 x 17 planes) ...
    want = {"nonfinite": {"rejected_centres": 100, "rejected_taps": 500, "all_taps_rejected": 3, "variance_skips": 20},
            "thresholds": {"sum_w_fallbacks": 3, "albedo_zeroed": 10, "background": 100},
            "black": {"black_waves": 50, "one_lane_waves": 8},
            "fireflies": {"firefly_clamps": 10, "f16_overflows": 1},
            "random": {"rejected_centres": 100, "clear_colour_selects": 100, "alpha_nan": 10, "firefly_clamps": 1}}[name]
    assert {k: total.get(k, 0) for k in want if total.get(k, 0) < want[k]} == {}, total
    # ... and at EVERY level, not only at level 0 (a level fed by the level before it sees finite values where that one skipped)
    per_level = {"nonfinite": {"rejected_centres": 3, "rejected_taps": 24, "all_taps_rejected": 3, "rejected_centre_and_all_taps": 1, "ff_count_zero": 2, "sum_w_fallbacks": 1},
                 "thresholds": {"rejected_centres": 1, "sum_w_fallbacks": 1},
                 "black": {"one_lane_waves": 2, "black_waves": 10}}.get(name, {})
    for level in range(4):
        assert {k: levels[level].get(k, 0) for k in per_level if levels[level].get(k, 0) < per_level[k]} == {}, (level, levels[level])


@pytest.mark.parametrize("mistake,name,kinds", [("transposed_kernel", "random", {"demodulation", "denoise"}), ("no_nan_skip", "nonfinite", {"denoise"}),
                                                ("firefly_on_channel_0", "fireflies", {"denoise"})])
def test_the_comparison_notices_a_planted_mistake(oracle, mistake, name, kinds):
    """Negative control: the reference run with the kernel index transposed, without the NaN skip and with the firefly test on
    channel 0 must each fail the comparison - the planes and the asymmetric kernel can tell."""
    planes = PP.make_planes(name, 7, PP.window_for((130, 17), 1.5), 1.5, 3, 3)
    *_, problems = check(planes, dispatches(oracle, planes, mistake=mistake), np.zeros_like(planes.placed))
    assert problems and {p.split(":")[0].split(" ")[0].rstrip("_l0123") for p in problems} >= kinds, problems


# ---------------------------------------------------------------- the shaders' own word: tests/golden/wgsl_post_planes_*.npz
def shader_fixture_cases():
    import os
    import sys

    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import wgsl_pin

    return wgsl_pin


def replay_planes(e, case):
    """tests/golden/wgsl_post_planes_<case>.npz holds what the REFERENCE'S SHADERS wrote in every dispatch of the post chain on the
    planes of `case` (tests/tools/wgsl_pin.py --planes --write, run where the reference is at hand).  Drive engine `e` through the
    same dispatches and return the (dispatch, buffer) whose bytes differ from what the shader wrote."""
    wgsl_pin = shader_fixture_cases()
    name, render_size, ratio, frame_number = case
    data = np.load(wgsl_pin.planes_fixture_path(*case))
    planes = PP.make_planes(name, 7, PP.window_for(render_size, ratio), ratio, 3, frame_number, compact=True)
    PP.install(e, planes)
    steps = [(p, ch) for ch in range(3) for p in (F.PASS_DEMODULATION, F.PASS_DENOISE_L0, F.PASS_DENOISE_L1, F.PASS_DENOISE_L2, F.PASS_DENOISE_L3)]
    bad, seen = [], 0
    for index, (pass_id, arg) in enumerate(steps + [(F.PASS_TONE_MAPPING, 1)], start=1):
        e.pass_run(pass_id, arg)
        for key in [k for k in data.files if int(k[1:4]) == index]:
            want = data[key]
            got = e.read(int(key.split("buf")[1])).view(np.uint8).reshape(-1)[:len(want)]
            seen += 1
            if not (got == want).all():
                bad.append((index, key, int((got != want).sum())))
    assert seen == len(data.files) == 15 * 6 + 1
    return bad


PLANES_FIXTURES = shader_fixture_cases().PLANES_FIXTURES


@pytest.mark.parametrize("case", PLANES_FIXTURES, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-f{c[3]}")
def test_oracle_equals_what_the_reference_shaders_wrote_on_the_planes(oracle, case):
    assert replay_planes(oracle, case) == []


@pytest.mark.skipif(not shader_fixture_cases().reference_available(), reason="no reference checkout (HIKARI_REFERENCE_DIR)")
@pytest.mark.parametrize("case", PLANES_FIXTURES, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-f{c[3]}")
def test_reference_shaders_reproduce_the_oracle_on_the_planes(case):
    """denoise.wgsl and tone_mapping.wgsl themselves, executed dispatch by dispatch on the oracle's state: byte for byte, the texels
    whose value WGSL leaves open included (the translator's runtime takes those choices from the numeric contract)."""
    wgsl_pin = shader_fixture_cases()
    results = wgsl_pin.run_planes(*case)
    assert len(results) == 16 and [r for r in results if r["mismatch"]] == []
    data = np.load(wgsl_pin.planes_fixture_path(*case))
    assert sorted(data.files) == sorted(wgsl_pin.run_planes.recorded)
    assert all((data[k] == wgsl_pin.run_planes.recorded[k]).all() for k in data.files)        # the committed fixture is what they write
