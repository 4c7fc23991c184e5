"""Known results (DESIGN 4 "Empty tiles"): the primary rays of a frame write one byte per 8x8 tile - 1 where all of them missed - and
the fused kernels of the same frame skip, for waves that lie in such tiles, the arithmetic that leads to the background's constants.
A context with HK_DEBUG_OPT_KNOWN_RESULTS at 0 takes the long way everywhere: the two must agree in every byte of every buffer, the plane
must say what the depth buffer says, and the launches must really have been handed it (or, where the rule forbids it, not)."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from cases import GBUFFER_IDS, diff_buffers, snapshot

pytestmark = pytest.mark.gpu

# 8x8 tiles, 64x1 row waves, 16x16 and 64x4 workgroups: a width of one wave and a tile more, sizes that are multiples of none of them
# but of 8, a single tile row of one wave, and two waves and a tile by 4.5 workgroups
SIZES = [(72, 40), (200, 136), (64, 8), (136, 72)]
RATIO_1 = hk.Upscale.SMAA_TU_1_0
# Emissive spatial reuse is on throughout: the camera moves, and a channel whose spatial pass is off keeps the reference's write-write
# race of the reprojected stores into previous_spatial (DESIGN 4 "The scatter race") - two contexts given the same frames may then
# differ in those records whatever this switch says.  With the pass on every store is resolved deterministically.
SETTINGS = {
    "denoise_b2": dict(indirect_bounces=2, emissive_spatial_reuse=True, denoise=True),
    "nodenoise_b0": dict(indirect_bounces=0, emissive_spatial_reuse=True, denoise=False),
    "denoise_b0": dict(indirect_bounces=0, emissive_spatial_reuse=True, denoise=True),
    "nodenoise_b2": dict(indirect_bounces=2, emissive_spatial_reuse=True, denoise=False),
}


def launches_per_frame(settings):
    """Every consumer of a frame, counted: the five fused light launches (sun, emissive, indirect, both spatial passes - all of them run
    with these settings, whatever the number of bounces) and, with the denoiser on, demodulation and the four a-trous levels.  The hook
    returns one total: asserting it EXACTLY says that each of them was handed the plane - demodulation, whose rule is the strictest
    (this frame's light passes over every row), included - and none twice."""
    return 5 + (5 if settings.denoise else 0)


def camera(view, w, h, step):
    """Cornell views; `step` moves the camera a little from frame to frame."""
    d = 0.04 * step
    if view == "centred":
        return hk.Camera(hk.look_at_transform((d, 1.0, 4.0), (d, 1.0, 0.0)), w, h)
    if view == "away":       # every primary ray misses
        return hk.Camera(hk.look_at_transform((d, 1.0, 4.0), (d, 1.0, 8.0)), w, h)
    if view == "inside":     # no primary ray misses
        return hk.Camera(hk.look_at_transform((0.2 * d, 1.0, 0.9), (0.2 * d, 1.0, -1.0)), w, h)
    if view == "rolled":     # the silhouette crosses the tile borders diagonally: the 3 x 3 neighbourhood of demodulation
        return hk.Camera(hk.look_at_transform((0.7 + d, 1.3, 4.5), (0.2 + d, 1.0, 0.0), up=(0.6, 0.8, 0.0)), w, h)
    raise KeyError(view)


@pytest.fixture(scope="module")
def pair():
    """(the library's default, HK_DEBUG_OPT_KNOWN_RESULTS 0): two contexts that are given the same frames throughout"""
    scene = hk.load_cornell()
    on, off = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    off.engine.set_debug_option(F.DEBUG_OPT_KNOWN_RESULTS, 0)
    for p in (on, off):
        p.set_scene(scene)
    return on, off


def empty_tiles_of_depth(engine):
    """numpy's own reading of the G-buffer: the 8x8 tiles (clipped at the image's edge) whose depths are all zero"""
    depth = engine.read(F.BUF_POSITION)[..., 3]
    h, w = depth.shape
    padded = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=np.float32)
    padded[:h, :w] = depth
    return (padded.reshape(padded.shape[0] // 8, 8, padded.shape[1] // 8, 8) == 0.0).all(axis=(1, 3)).astype(np.uint8)


def render_sequence(pair, view, w, h, settings, first, frames=4):
    """`frames` frames enqueued without a read in between, the camera moving; returns the launches the default context was handed the plane in"""
    on, off = pair
    for p in pair:
        if p._size != (w, h, 1.0):
            p.engine.resize(w, h, 1.0)
            p._size = (w, h, 1.0)
    before = on.engine.empty_tiles()[1]
    for k in range(frames):
        for p in pair:
            p.render(camera(view, w, h, first + k), settings, frame_number=first + k)
    tiles, after = on.engine.empty_tiles()
    assert off.engine.empty_tiles()[1] == 0   # the switch: no launch of that context ever sees a plane
    return tiles, after - before


def assert_same_bytes(pair, what):
    on, off = pair
    bad = diff_buffers(snapshot(on), snapshot(off))
    assert bad == {}, (what, bad)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_buffer_equals_the_long_way(pair, size):
    w, h = size
    n = 1
    for name, kw in SETTINGS.items():
        s = hk.HikariSettings(upscale=RATIO_1, **kw)
        for view in ("centred", "away", "inside", "rolled"):
            for p in pair:   # (a fresh history per case: reallocated and zeroed, light.rs:342-363)
                p.engine.resize(w, h, 1.0)
                p._size = (w, h, 1.0)
                p._previous_camera = None
            tiles, launches = render_sequence(pair, view, w, h, s, n)
            n += 4
            want = empty_tiles_of_depth(pair[0].engine)
            assert (tiles == want).all(), (name, view, tiles, want)
            if view == "away":
                assert (want == 1).all()
            elif view == "inside":
                assert (want == 0).all(), want
            elif h >= 40:   # (the box in the middle of the image, background around it)
                assert 0 < want.sum() < want.size, (view, want)
            assert launches == 4 * launches_per_frame(s), (name, view, launches)
            assert_same_bytes(pair, (name, view, size))


def test_ratio_other_than_one_keeps_the_long_way(pair):
    s = hk.HikariSettings(indirect_bounces=2, emissive_spatial_reuse=True, upscale=hk.Upscale.Fsr1(1.5, 0.2))
    on, off = hk.HikariPlugin(device=0), pair[1]
    on.set_scene(hk.load_cornell())
    off._size = off._previous_camera = None   # (as the fresh context: the first frame resizes, no previous view)
    for view in ("centred", "away"):
        for k in range(4):
            for p in (on, off):
                p.render(camera(view, 136, 72, k), s, frame_number=k + 1)
        assert on.engine.empty_tiles()[1] == 0
        assert_same_bytes((on, off), ("ratio 1.5", view))


def test_host_rasterised_gbuffer_keeps_the_long_way(pair):
    """hk_frame_begin, the five planes written with hk_write_buffer, hk_frame_render(HK_FRAME_EXTERNAL_GBUFFER): the plane of these frames
    was written by nobody"""
    w, h = 72, 40
    s = hk.HikariSettings(indirect_bounces=2, emissive_spatial_reuse=True, upscale=RATIO_1)
    source, on, off = pair[0], hk.HikariPlugin(device=0), pair[1]
    on.set_scene(hk.load_cornell())
    lights = hk.lights_uniform()
    for p in (on, off):
        p.engine.resize(w, h, 1.0)
        p._size = (w, h, 1.0)
    for n in (1, 2, 3):
        cam = camera("centred", w, h, n)
        source.render(cam, s, frame_number=n)
        planes = [source.engine.read(b) for b in GBUFFER_IDS]
        frame, view, pview = hk.frame_uniform(s, n), cam.view_uniform(), cam.previous_view_uniform()
        for p in (on, off):
            p.engine.frame_begin(frame, view, pview, lights)
            for b, plane in zip(GBUFFER_IDS, planes):
                p.engine.write(b, plane)
            p.engine.frame_render(frame, view, pview, lights, s.to_c(), F.FRAME_EXTERNAL_GBUFFER)
    assert on.engine.empty_tiles()[1] == 0
    assert_same_bytes((on, off), "external G-buffer")


def test_write_buffer_between_two_frames(pair):
    """a host write into the position plane: the frame after it gets no plane (and renders what the long way renders), the one after that does again"""
    w, h = 136, 72
    s = hk.HikariSettings(indirect_bounces=2, emissive_spatial_reuse=True, upscale=RATIO_1)
    on, off = pair
    for p in pair:   # (the same frames for both: a fresh history and no previous view, whatever the tests before left behind)
        p.engine.resize(w, h, 1.0)
        p._size = (w, h, 1.0)
        p._previous_camera = None
    _, launches = render_sequence(pair, "rolled", w, h, s, 1, frames=2)
    assert launches == 2 * launches_per_frame(s)
    assert_same_bytes(pair, "before hk_write_buffer")
    position = on.engine.read(F.BUF_POSITION)
    position[: h // 2] = 0.0   # (the top half of the image turned into background behind the primary rays' back)
    for p in pair:
        p.engine.write(F.BUF_POSITION, position)
    _, launches = render_sequence(pair, "rolled", w, h, s, 3, frames=1)
    assert launches == 0
    assert_same_bytes(pair, "the frame after hk_write_buffer")
    _, launches = render_sequence(pair, "rolled", w, h, s, 4, frames=1)
    assert launches == launches_per_frame(s)
    assert_same_bytes(pair, "the second frame after hk_write_buffer")
