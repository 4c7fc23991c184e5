"""Background stores (DESIGN 4 "Empty tiles"): a wave whose tile was empty in the last frame of its parity and is empty again skips the
stores that would rewrite the background's constants - the primary rays their eight planes, the direct-light kernels and the spatial
passes variance / render.  A context with HK_DEBUG_OPT_KNOWN_RESULTS at 0 stores everything: given the same frames the two must agree in
every byte of every buffer after EVERY frame - through sequences in which both parities are granted and lose the grant, and across each
event that must end it (the garbage a host writes into a plane has to be gone from both contexts alike)."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from cases import GBUFFER_IDS, diff_buffers, product_default_plugin, snapshot

pytestmark = pytest.mark.gpu

# two waves and a tile by 4.5 workgroups; a wave and a tile; tiles clipped at both edges
SIZES = [(136, 72), (72, 40), (75, 43)]
RATIO_1 = hk.Upscale.SMAA_TU_1_0
# (emissive spatial reuse on: a channel whose spatial pass is off keeps the reference's scatter race - tests/test_known_results_gpu.py)
BASE = dict(indirect_bounces=2, emissive_spatial_reuse=True, denoise=True)


def settings(**kw):
    return hk.HikariSettings(upscale=RATIO_1, **{**BASE, **kw})


def camera(view, w, h):
    if view == "centred":    # the box in the middle, background around it
        return hk.Camera(hk.look_at_transform((0.0, 1.0, 4.0), (0.0, 1.0, 0.0)), w, h)
    if view == "panned":     # the box at the left edge: tiles that held it are empty, tiles that were empty hold it
        return hk.Camera(hk.look_at_transform((0.0, 1.0, 4.0), (1.6, 1.3, 0.0)), w, h)
    if view == "away":       # every primary ray misses
        return hk.Camera(hk.look_at_transform((0.0, 1.0, 4.0), (0.0, 1.0, 8.0)), w, h)
    raise KeyError(view)


def make_pair(make):
    scene = hk.load_cornell()
    on, off = make(), make()
    off.engine.set_debug_option(F.DEBUG_OPT_KNOWN_RESULTS, 0)
    for p in (on, off):
        p.set_scene(scene)
    return on, off


@pytest.fixture(scope="module")
def pair():
    """(the library's default, HK_DEBUG_OPT_KNOWN_RESULTS 0), with the suite's HK_CTX_EXACT_TRAVERSAL"""
    return make_pair(lambda: hk.HikariPlugin(device=0))


@pytest.fixture(scope="module")
def product_pair():
    """... and as bench.py runs them: the one-level walk from LDS, whose instantiations are the headline's"""
    return make_pair(product_default_plugin)


def fresh(pair, w, h):
    for p in pair:   # (reallocated and zeroed: no grant, no history, no previous view)
        p.engine.resize(w, h, 1.0)
        p._size = (w, h, 1.0)
        p._previous_camera = None


def frame(pair, view, w, h, s, n, what):
    """one frame for both contexts, then every buffer compared"""
    on, off = pair
    for p in pair:
        p.render(camera(view, w, h), s, frame_number=n)
    bad = diff_buffers(snapshot(on), snapshot(off))
    assert bad == {}, (what, "frame", n, view, bad)


SEQUENCES = {
    # (view, frame number) per frame
    "away": [("away", n) for n in range(1, 8)],
    "centred": [("centred", n) for n in range(1, 8)],
    # tiles turn from empty to geometry and back, on both parities, with kept frames in between
    "pan": list(zip(["centred", "centred", "centred", "panned", "panned", "panned", "panned", "centred", "panned", "centred", "centred", "away", "centred", "centred"],
                    range(1, 15))),
    # two frames of one parity in a row (the planes do not flip: the last writer is the previous frame)
    "same_parity": list(zip(["centred", "centred", "centred", "panned", "panned", "centred", "centred", "centred", "panned", "panned"], [1, 2, 3, 5, 7, 8, 10, 12, 13, 14])),
}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_every_frame_equals_the_long_way(pair, size, name):
    w, h = size
    fresh(pair, w, h)
    for view, n in SEQUENCES[name]:
        frame(pair, view, w, h, settings(), n, name)
    assert pair[0].engine.empty_tiles()[1] > 0 and pair[1].engine.empty_tiles()[1] == 0


@pytest.mark.parametrize("name", ["pan", "same_parity"])
def test_the_headline_instantiations_equal_the_long_way(product_pair, name):
    w, h = 75, 43
    fresh(product_pair, w, h)
    for view, n in SEQUENCES[name]:
        frame(product_pair, view, w, h, settings(), n, ("product default", name))


def garbage(pair, buf):
    """the same non-zero bytes into one plane of both contexts (0x3f3f...: finite in f32 and f16)"""
    for p in pair:
        plane = p.engine.read(buf).copy()
        plane.view(np.uint8)[...] = 0x3F
        p.engine.write(buf, plane)


def external_gbuffer_frame(pair, w, h, n):
    """frame n with a G-buffer the host wrote (the planes of the frame before, as good as any)"""
    s = settings()
    cam = camera("centred", w, h)
    planes = [pair[1].engine.read(b) for b in GBUFFER_IDS]
    lights = hk.lights_uniform()
    for p in pair:
        fr, view, pview = hk.frame_uniform(s, n), cam.view_uniform(), cam.previous_view_uniform(p._previous_camera)
        p.engine.frame_begin(fr, view, pview, lights)
        for b, plane in zip(GBUFFER_IDS, planes):
            p.engine.write(b, plane)
        p.engine.frame_render(fr, view, pview, lights, s.to_c(), F.FRAME_EXTERNAL_GBUFFER)
        p._previous_camera = cam


def resize_and_back(pair, w, h):
    for p in pair:
        p.engine.resize(w + 16, h + 8, 1.0)
        p.engine.resize(w, h, 1.0)
        p._previous_camera = None


def hand_driven(pair, passes):
    for p in pair:
        for pass_id in passes:
            p.engine.pass_run(pass_id)


# what happens between frame 6 and frame 7 of a running static sequence: (event, settings of the frames after it)
EVENTS = {
    "write_position": (lambda pair, w, h: garbage(pair, F.BUF_POSITION), {}),
    "write_velocity_uv": (lambda pair, w, h: garbage(pair, F.BUF_VELOCITY_UV), {}),
    "write_previous_position": (lambda pair, w, h: garbage(pair, F.BUF_PREVIOUS_POSITION), {}),
    "write_albedo": (lambda pair, w, h: garbage(pair, F.BUF_ALBEDO), {}),
    "write_render": (lambda pair, w, h: garbage(pair, F.BUF_RENDER0 + 1), {}),
    "write_variance": (lambda pair, w, h: garbage(pair, F.BUF_VARIANCE0), {}),
    "write_denoise_internal": (lambda pair, w, h: garbage(pair, F.BUF_DENOISE_INTERNAL0 + 1), {}),
    "write_tone_mapped": (lambda pair, w, h: garbage(pair, F.BUF_TONE_MAPPED), {}),
    "resize_and_back": (resize_and_back, {}),
    "external_gbuffer": (lambda pair, w, h: external_gbuffer_frame(pair, w, h, 7), {}),
    "pass_run_light": (lambda pair, w, h: hand_driven(pair, [F.PASS_DIRECT_LIT, F.PASS_EMISSIVE_SPATIAL_REUSE]), {}),
    "pass_run_prepass": (lambda pair, w, h: hand_driven(pair, [F.PASS_PREPASS]), {}),
    "pass_run_denoise": (lambda pair, w, h: hand_driven(pair, [F.PASS_DENOISE_L1]), {}),
    "denoise_off": (None, dict(denoise=False)),
    "bounces_0": (None, dict(indirect_bounces=0)),
    "clear_colour": (None, dict(clear_color=(0.1, 0.7, 0.2, 1.0))),
}


@pytest.mark.parametrize("size", [(72, 40), (75, 43)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(EVENTS))
def test_event_ends_the_grant(pair, size, name):
    """six static frames (both parities kept), the event, frames after it - two of them with the changed settings where the event is a
    setting, then the first settings again: every buffer after every frame"""
    w, h = size
    event, changed = EVENTS[name]
    fresh(pair, w, h)
    for n in range(1, 7):
        frame(pair, "centred", w, h, settings(), n, (name, "before"))
    first = 7
    if event:
        event(pair, w, h)
        if name == "external_gbuffer":
            bad = diff_buffers(snapshot(pair[0]), snapshot(pair[1]))
            assert bad == {}, (name, "the external frame", bad)
            first = 8
    for n in range(first, first + 6):
        s = settings(**changed) if n < first + 2 else settings()
        frame(pair, "centred", w, h, s, n, (name, "after"))


def test_ratio_other_than_one_in_between(pair):
    w, h = 72, 40
    fresh(pair, w, h)
    for n in range(1, 7):
        frame(pair, "centred", w, h, settings(), n, "before ratio 1.5")
    s15 = hk.HikariSettings(upscale=hk.Upscale.Fsr1(1.5, 0.2), **BASE)
    for p in pair:   # (the plugin resizes for the ratio, and back for the frames after)
        p.render(camera("centred", w, h), s15, frame_number=7)
    bad = diff_buffers(snapshot(pair[0]), snapshot(pair[1]))
    assert bad == {}, ("the ratio-1.5 frame", bad)
    for n in range(8, 14):
        frame(pair, "centred", w, h, settings(), n, "after ratio 1.5")
