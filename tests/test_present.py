"""tests/present_ref.py - the numpy restatement hk_present is held to on the GPU - against an independent float64 formulation of the
same steps, on the adversarial planes of the GPU tests.  No GPU.

Tolerance (u = 2^-24, one f32 rounding).  Every step of the reference is a short chain of f32 operations on exact f16 inputs, so a
running first-order bound is carried beside the float64 value, with |.| propagated through the same formulas:
  sampling   the bilinear blend is a 4-term sum  t00 (1-fx)(1-fy) + t10 fx (1-fy) + t01 (1-fx) fy + t11 fx fy.  Each term passes
             through at most 6 roundings in `mix(mix(..), mix(..), fy)` (1-fx, the product, the inner sum, 1-fy, the product,
             the outer sum); the fractions carry 3 more (the division, the scale by the plane's size n, the -0.5, each at most
             u * n absolute; the subtraction of the floor is exact) and multiply the texel DIFFERENCES along their axis.
             err_c <= 6u * sum |t| w + 3u * n_x * (|t10 - t00| + |t11 - t01|) + 3u * n_y * (|t01 - t00| + |t11 - t10|).
             A plane read at the texel is exact.
  HDR        l = fma chain: 3 roundings on sum |c| k, plus the sampling error through the weights;  s = l'/(1-l') / l has 3 more
             roundings and the derivative  |ds/dl| = |s| / (1-l') inside the clamp, |s| / |l| outside it (their sum where l is
             within its error of a clamp edge);  rgb * s one more.
  blend      c a + d (1-a): at most 3 roundings per term (1-a, the product, the sum) on |c a| + |d (1-a)|, plus the errors of c, a and (for a decoded target) nothing: d is exact.
  encode     sRGB: the slope of the curve (<= 12.92) times the error above, plus pow_'s own error - 4 ulp of the result, the
             bound tests/test_math_contract.py holds it to on this range - plus 2 roundings.
The bound is first order; a factor 1 + 2^-8 covers the second-order terms (every relative error involved is < 2^-10 where the
bound is used - texels whose luminance is cancelled to within 2^-10 of its terms are compared by class only, and counted).
Non-finite float64 results (a black texel's 0 * inf under HDR, inf - inf, a NaN albedo) must be non-finite in the reference.
8-bit codes may differ by one, and only where the float64 value lies within the bound of a rounding boundary."""
import os

import numpy as np
import pytest

import present_ref as R

U = 2.0 ** -24
CLEAR = (0.125, 0.25, 0.5, 0.75)
BY_CLASS_SHARE = {"equal": 0.02, "upscaled": 0.05, "albedo-differs": 0.03}   # see test_the_reference_agrees_with_float64
CASES = {"equal": ((37, 19), (37, 19), (37, 19)), "upscaled": ((24, 13), (37, 19), (37, 19)), "albedo-differs": ((24, 13), (48, 26), (24, 13))}


def sample64(plane_u16, W, H):
    """-> (value, error bound) in float64"""
    t = plane_u16.view(np.float16).astype(np.float64)
    h, w = t.shape[:2]
    if (w, h) == (W, H):
        return t, np.zeros_like(t)

    def axis(n_out, n_in):
        p = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
        i = np.floor(p).astype(np.int64)
        return np.clip(i, 0, n_in - 1), np.clip(i + 1, 0, n_in - 1), p - np.floor(p)

    x0, x1, fx = axis(W, w)
    y0, y1, fy = axis(H, h)
    fx, fy = fx[None, :, None], fy[:, None, None]
    with np.errstate(all="ignore"):
        terms = [(t[y0][:, x0], (1 - fx) * (1 - fy)), (t[y0][:, x1], fx * (1 - fy)), (t[y1][:, x0], (1 - fx) * fy), (t[y1][:, x1], fx * fy)]
        value = sum(a * wgt for a, wgt in terms)
        mag = sum(np.abs(a) * wgt for a, wgt in terms)
        (t00, _), (t10, _), (t01, _), (t11, _) = terms
        dx, dy = np.abs(t10 - t00) + np.abs(t11 - t01), np.abs(t01 - t00) + np.abs(t11 - t10)   # what an error of fx / fy multiplies
        return value, 6 * U * mag + 3 * U * w * dx + 3 * U * h * dy


def present64(src, albedo, W, H, hdr, d):
    """-> (linear output before the encode, error bound, texels compared by class only)"""
    with np.errstate(all="ignore"):
        c, ec = sample64(src, W, H)
        bad = np.isnan(c).any(axis=-1)
        ca, eca = sample64(albedo, W, H)
        c, ec = np.where(bad[..., None], ca, c), np.where(bad[..., None], eca, ec)
        loose = np.zeros((H, W), dtype=bool)
        if hdr:
            k = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], dtype=np.float64)
            rgb, ergb = c[..., :3], ec[..., :3]
            lum, labs = (rgb * k).sum(-1), (np.abs(rgb) * k).sum(-1)
            el = 3 * U * labs + (ergb * k).sum(-1)
            lo, hi = float(np.float32(0.0005)), float(np.float32(0.995))
            l_old = np.fmin(np.fmax(lum, lo), hi)
            s = l_old / (1.0 - l_old) / lum
            inside, at_edge = (lum > lo) & (lum < hi), (np.abs(lum - lo) <= el) | (np.abs(lum - hi) <= el)
            slope = np.where(at_edge, 1.0 / (1.0 - l_old) + 1.0 / np.abs(lum), np.where(inside, 1.0 / (1.0 - l_old), 1.0 / np.abs(lum)))
            es = np.abs(s) * (3 * U + el * slope)
            loose = ~(el < 2.0 ** -10 * np.abs(lum))
            out_rgb = rgb * s[..., None]
            e_rgb = np.abs(out_rgb) * U + np.abs(s)[..., None] * ergb + np.abs(rgb) * es[..., None]
            c, ec = np.concatenate([out_rgb, c[..., 3:]], -1), np.concatenate([e_rgb, ec[..., 3:]], -1)
        a, ea = c[..., 3:], ec[..., 3:]
        kk = 1.0 - a
        o = np.concatenate([c[..., :3] * a + d[..., :3] * kk, a + d[..., 3:] * kk], -1)
        mag = np.concatenate([np.abs(c[..., :3] * a) + np.abs(d[..., :3] * kk), np.abs(a) + np.abs(d[..., 3:] * kk)], -1)
        e = 3 * U * mag + np.concatenate([np.abs(a) * ec[..., :3] + (np.abs(c[..., :3]) + np.abs(d[..., :3])) * ea, (1 + np.abs(d[..., 3:])) * ea], -1)
        return o, (1.0 + 2.0 ** -8) * e, loose


def encode64(v):
    with np.errstate(all="ignore"):
        return np.where(v <= float(np.float32(0.0031308)), 12.92 * v, 1.055 * np.power(np.maximum(v, 0.0), 1.0 / 2.4) - 0.055)


def compare(name, fmt, hdr, clear):
    """-> (texels checked against the bound, components near a code boundary, components compared by class only, failures)"""
    src_size, albedo_size, (W, H) = CASES[name]
    src, albedo = R.make_planes(src_size, albedo_size)
    before = R.random_target(fmt, W, H)
    ref = R.present(src, albedo, W, H, fmt, hdr=hdr, clear=clear, target=before)
    d = np.broadcast_to(np.asarray(clear, np.float32).astype(np.float64), (H, W, 4)) if clear is not None else R.decode(before, fmt).astype(np.float64)
    o, e, loose = present64(src, albedo, W, H, hdr, d)
    finite = np.isfinite(o) & np.isfinite(e) & ~loose[..., None]
    fails = []
    if fmt in ("rgba16f", "rgba32f"):
        got = ref.astype(np.float64)
        if (np.isfinite(got) & ~np.isfinite(o) & ~loose[..., None]).any():
            fails.append("finite where float64 is not")
        tol = e + U * np.abs(o)
        if fmt == "rgba16f":   # + the f16 rounding of the store: half an ulp (2^-11 relative, 2^-25 for denormals), overflow to inf above 65504
            tol = tol + np.maximum(np.abs(o) * 2.0 ** -11, 2.0 ** -25)
            finite &= np.abs(o) + tol < 65504.0
        with np.errstate(all="ignore"):
            wrong = finite & ~(np.abs(got - o) <= tol)
        if wrong.any():
            fails.append(("beyond the bound", int(wrong.sum()), float(np.nanmax(np.where(wrong, np.abs(got - o) / tol, 0)))))
        return int(finite.sum()), 0, int((~finite).sum()), fails
    order = [2, 1, 0, 3] if fmt == "bgra8-srgb" else [0, 1, 2, 3]
    codes = ref[..., order].astype(np.int64)          # rgba order
    enc = np.concatenate([encode64(o[..., :3]), o[..., 3:]], -1)
    with np.errstate(all="ignore"):
        slope = np.where(o[..., :3] <= 0.0031308, 12.92, np.minimum(12.92, (1.055 / 2.4) * np.power(np.maximum(o[..., :3], 1e-30), 1.0 / 2.4 - 1.0)))
        ee = np.concatenate([slope * e[..., :3] + 6 * U * np.maximum(np.abs(enc[..., :3]), 0.055), e[..., 3:]], -1) + 2 * U
        scaled = 255.0 * np.clip(enc, 0.0, 1.0)
        want = np.floor(0.5 + scaled).astype(np.int64)
        # within the bound of a boundary k + 0.5: the two ends of [enc - ee, enc + ee] round to different codes (after the clamp - a value
        # far outside [0, 1] is code 0 or 255 whatever its error)
        lo, hi = 255.0 * np.clip(enc - ee, 0.0, 1.0) - 256 * U, 255.0 * np.clip(enc + ee, 0.0, 1.0) + 256 * U
        near = np.floor(0.5 + lo) != np.floor(0.5 + hi)
    nonfinite = ~finite
    want = np.where(np.isnan(enc), 0, want)           # clamp_(NaN) = 0
    check = ~nonfinite | np.isnan(enc) & ~loose[..., None]
    diff = np.abs(codes - want)
    if (check & (diff > 1)).any():
        fails.append(("codes more than one apart", int((check & (diff > 1)).sum())))
    if (check & (diff == 1) & ~near).any():
        fails.append(("codes differ away from a boundary", int((check & (diff == 1) & ~near).sum())))
    return int(check.sum()), int((check & near).sum()), int((~check).sum()), fails


@pytest.mark.parametrize("name", list(CASES))
def test_the_reference_agrees_with_float64(name):
    checked = near = by_class = total = 0
    fails = {}
    for fmt in R.FORMATS:
        for hdr in (False, True):
            for clear in (CLEAR, None):
                n, b, c, f = compare(name, fmt, hdr, clear)
                if fmt.endswith("srgb"):
                    checked, near = checked + n, near + b
                by_class += c
                total += CASES[name][2][0] * CASES[name][2][1] * 4
                if f:
                    fails[(fmt, hdr, clear is not None)] = f
    print(f"{name}: {by_class} of {total} components by class only ({100.0 * by_class / total:.2f} %)")
    print(f"{name}: {checked} 8-bit components checked, {near} within the bound of a code boundary ({100.0 * near / checked:.3f} %), {by_class} components compared by class only")
    assert fails == {}
    # compared by class only (non-finite in float64, or a luminance cancelled to within 2^-10 of its terms): the specials of the planes
    # and their bilinear footprints.  Measured, of all components of the 16 combinations: equal 0.64 %, upscaled 2.98 %, albedo-differs
    # 1.44 % (about ten non-finite texels of the plane, times the nine target pixels a bilinear footprint spreads each over); the caps
    # are about twice that - the bound must not become vacuous by this set growing
    assert by_class < BY_CLASS_SHARE[name] * total
    assert near < 0.01 * checked     # measured on these planes: equal 0.64 %, upscaled 0.22 %, albedo-differs 0.41 %


def test_the_planes_hold_what_they_promise():
    src, albedo = R.make_planes((24, 13), (37, 19))
    t = src.view(np.float16).astype(np.float32)
    nan = np.isnan(t)
    assert (nan.sum(-1) <= 1).all() and all(nan[..., k].sum() == 1 for k in range(4))           # one NaN per channel, each alone
    assert np.isnan(albedo.view(np.float16)).any() and np.isnan(albedo.view(np.float16)[0, 0]).any() and nan[0, 0].any()
    assert np.isposinf(t).any() and np.isneginf(t).any() and (t < 0).any() and (t == 65504).any()
    assert (src == R.H_NZERO).any() and (src == 0).any() and (src == R.H_DENORMAL).any()
    alphas = set(np.unique(src[..., 3]))
    assert {0, R.H_DENORMAL, int(R.f16(0.5)), int(R.f16(1.0)), int(R.f16(2.0))} <= alphas
    assert ((src[..., :3] == 0).all(-1) & (src[..., 3] == int(R.f16(1.0)))).any()                # black, alpha 1
    b = set(int(v) for v in R.srgb_boundaries())
    assert len(b) == 256 and b <= set(int(v) for v in src[..., :3].ravel())


def test_the_decode_table_is_the_encodes_inverse():
    """every 8-bit code survives decode -> encode (the table the material textures use against the curve the present encodes with)"""
    codes = np.arange(256, dtype=np.uint8)
    assert (R.unorm8_code(R.srgb_encode(R.SRGB_LUT[codes])) == codes).all()


# ---------------------------------------------------------------------------------------------- the HDR step from the shader text
HDR_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgsl_overlay_hdr_4096.npz")


def hdr_colours():
    """4 096 colours for `inverse_reintard_luminance`: the f16 specials of the planes in every channel, colours whose luminance sits
    on and next to both clamp edges, black, cancelling negative channels, and seeded f16 colours over the image's range"""
    rng = np.random.default_rng(17)
    special = np.array([0.0, -0.0, 6e-8, 0.0005, 0.995, 1.0, 65504.0, -0.25, np.inf, -np.inf, np.nan, 0.5], dtype=np.float32)
    grid = np.stack(np.meshgrid(special, special, special, indexing="ij"), -1).reshape(-1, 3)                      # 1 728
    edges = []
    for target in (0.0005, 0.995):
        for ulps in range(-8, 9):
            g = np.float32(target) + np.float32(ulps) * np.spacing(np.float32(target))
            edges += [[g, g, g], [g / np.float32(0.2126), 0.0, 0.0], [0.0, g / np.float32(0.7152), 0.0], [0.0, 0.0, g / np.float32(0.0722)]]
    edges = np.array(edges, dtype=np.float32)                                                                      # 136
    cancel = np.array([[1.0, -0.29726, 0.0], [-3.364, 1.0, 0.0], [0.25, 0.25, -3.213]], dtype=np.float32)
    n = 4096 - len(grid) - len(edges) - len(cancel)
    rand = (rng.random((n, 3)) ** 3 * 4.0).astype(np.float16).astype(np.float32)
    rand[: n // 8] *= np.float32(1e-3)
    return np.ascontiguousarray(np.concatenate([grid, edges, cancel, rand]), dtype=np.float32)


def shader_hdr(colours):
    """overlay.wgsl's `inverse_reintard_luminance` as the reference's text has it, executed through tests/tools/wgsl"""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import wgsl_pin
    from wgsl import engine, runtime, translate
    from wgsl import types as T

    mods = engine.library(wgsl_pin.SHADERS)
    extra = engine._split_modules(os.path.join(os.path.dirname(engine.__file__), "bevy_0_9_1_change_luminance.wgsl"))
    assert list(extra) == ["bevy_core_pipeline::tonemapping"]
    mods["bevy_core_pipeline::tonemapping"] += extra["bevy_core_pipeline::tonemapping"]
    source = engine.preprocess(open(os.path.join(wgsl_pin.SHADERS, "overlay.wgsl")).read(), {"HDR"}, mods)
    ns = {"_R": runtime, "_T": T, "RESOURCES": {}, "WORKGROUP_VARS": {}, "ENTRY_POINTS": {}, "_ONCE": (0,)}
    exec(compile(translate.translate(source), "<wgsl:overlay.wgsl>", "exec"), ns)
    fn = ns[translate.pyname("inverse_reintard_luminance")]
    out = np.empty_like(colours)
    with np.errstate(all="ignore"):
        for i, c in enumerate(colours):
            out[i] = [np.float32(v) for v in fn(runtime.V(np.float32(v) for v in c))]
    return out


def same_f32(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def hdr_of_reference(colours):
    rgba = np.concatenate([colours, np.ones((len(colours), 1), np.float32)], -1)
    return np.ascontiguousarray(R.hdr_step(rgba)[..., :3])


@pytest.mark.skipif(not os.path.isdir("/root/reference") and not os.environ.get("HIKARI_REFERENCE_DIR"), reason="no reference checkout")
def test_the_hdr_step_equals_the_shader_text_bit_for_bit():
    """`present_ref.hdr_step` against overlay.wgsl's own `inverse_reintard_luminance` (with bevy's `tonemapping_change_luminance`
    from tests/tools/wgsl/bevy_0_9_1_change_luminance.wgsl) on 4 096 colours, and the committed fixture against both."""
    colours = hdr_colours()
    assert colours.shape == (4096, 3)
    got = shader_hdr(colours)
    assert same_f32(got, hdr_of_reference(colours))
    fixture = np.load(HDR_FIXTURE)
    assert same_f32(fixture["colours"], colours) and same_f32(fixture["shader_output"], got)


def test_the_hdr_step_equals_what_the_shader_wrote():
    """the same pin without a reference checkout: the committed inputs and the outputs the shader text produced for them"""
    fixture = np.load(HDR_FIXTURE)
    assert fixture["colours"].shape == (4096, 3) and same_f32(fixture["colours"], hdr_colours())
    out = fixture["shader_output"]
    assert np.isnan(out).any() and np.isfinite(out).all(-1).sum() > 2000          # black / NaN colours and ordinary ones
    assert same_f32(hdr_of_reference(fixture["colours"]), out)
