"""Post stores (DESIGN 4 "Empty tiles"): demodulation and the a-trous levels skip their constant stores in tiles that were empty in the
frame before this one and are empty again (HK_TILE_POST_KEPT) - their planes are written by every frame - and level 3 skips the
tone-mapped image, which is twinned by frame parity, only where the tile was empty in the last frame of this parity as well.  A context
with HK_DEBUG_OPT_KNOWN_RESULTS at 0 stores everything: given the same frames the two must agree in every byte of every buffer
after EVERY frame - through static views, tiles that become empty and stop being empty, a tile that is empty in frames n - 2 and n but
not in n - 1, and across each event that must end the grant (the garbage a host writes into a plane has to be gone from both alike)."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from cases import diff_buffers, product_default_plugin, snapshot
from test_background_stores_gpu import camera, fresh, hand_driven, make_pair, resize_and_back, settings

pytestmark = pytest.mark.gpu

# a partial second wave per row of 64 pixels; several row-waves, each across eight tiles of mixed state
SIZES = [(75, 43), (200, 43)]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]


@pytest.fixture(scope="module")
def pair():
    """(the library's default, HK_DEBUG_OPT_KNOWN_RESULTS 0), with the suite's HK_CTX_EXACT_TRAVERSAL"""
    return make_pair(lambda: hk.HikariPlugin(device=0))


@pytest.fixture(scope="module")
def product_pair():
    """... and as bench.py runs them: the one-level walk from LDS, whose instantiations are the headline's"""
    return make_pair(product_default_plugin)


def compare(pair, what):
    bad = diff_buffers(snapshot(pair[0]), snapshot(pair[1]))
    assert bad == {}, (what, bad)


def frame(pair, view, w, h, s, n, what, staged=False, post=True):
    """one frame for both contexts - through hk_frame_render, or stage by stage (post=False: without its post stage) - then every buffer"""
    for p in pair:
        if not staged:
            p.render(camera(view, w, h), s, frame_number=n)
            continue
        cam = camera(view, w, h)
        p.engine.frame_begin(hk.frame_uniform(s, n), cam.view_uniform(), cam.previous_view_uniform(p._previous_camera), hk.lights_uniform())
        for stage in (F.STAGE_TEMPORAL, F.STAGE_SPATIAL) + ((F.STAGE_POST_PROCESS,) if post else ()):
            p.engine.frame_stage(stage, s.to_c())
        p._previous_camera = cam
    compare(pair, (what, "frame", n, view))


SEQUENCES = {
    "static": [("centred", n) for n in range(1, 9)],
    "away": [("away", n) for n in range(1, 8)],
    # tiles turn from empty to geometry and back on both parities: a tile that is newly empty in frame n - 1 holds frame n - 2's geometry in
    # this parity's tone-mapped plane, while the planes every frame writes hold their constants already
    "pan": list(zip(["centred", "centred", "centred", "panned", "panned", "panned", "panned", "centred", "panned", "centred", "centred", "away", "centred", "centred"],
                    range(1, 15))),
    # the gap: tiles empty in frames n - 2 and n (HK_TILE_KEPT) but not in n - 1 must store in n - on either parity
    "gap": list(zip(["centred", "centred", "centred", "centred", "panned", "centred", "centred", "panned", "centred", "panned", "centred", "centred"], range(1, 13))),
    # two frames of one parity in a row: the frame before is not the other parity's
    "same_parity": list(zip(["centred", "centred", "centred", "centred", "centred", "panned", "centred", "centred", "centred"], [1, 2, 3, 4, 6, 8, 9, 10, 11])),
    # the same frame number twice, with another view the second time
    "number_twice": list(zip(["centred", "centred", "centred", "centred", "panned", "centred", "centred", "centred"], [1, 2, 3, 4, 4, 5, 6, 7])),
}


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_every_frame_equals_the_long_way(pair, size, name):
    w, h = size
    fresh(pair, w, h)
    for view, n in SEQUENCES[name]:
        frame(pair, view, w, h, settings(), n, name)
    assert pair[0].engine.empty_tiles()[1] > 0 and pair[1].engine.empty_tiles()[1] == 0


@pytest.mark.parametrize("name", ["pan", "gap"])
def test_the_headline_instantiations_equal_the_long_way(product_pair, name):
    w, h = 75, 43
    fresh(product_pair, w, h)
    for view, n in SEQUENCES[name]:
        frame(product_pair, view, w, h, settings(), n, ("product default", name))


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_stages_driven_one_by_one(pair, size):
    """... through hk_frame_stage; frame 7 without its post stage (frame 8's chain then follows frame 6's), frame 10 rendered whole"""
    w, h = size
    fresh(pair, w, h)
    views = ["centred"] * 6 + ["panned", "panned", "centred", "centred", "centred", "centred"]
    for n, view in enumerate(views, start=1):
        frame(pair, view, w, h, settings(), n, "staged", staged=n != 10, post=n != 7)


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_without_frame_pipelining(pair, size):
    w, h = size
    fresh(pair, w, h)
    for p in pair:
        p.engine.set_debug_option(F.DEBUG_OPT_FRAME_PIPELINE, 0)
    try:
        for view, n in SEQUENCES["gap"]:
            frame(pair, view, w, h, settings(), n, "HK_DEBUG_OPT_FRAME_PIPELINE 0")
    finally:
        for p in pair:
            p.engine.set_debug_option(F.DEBUG_OPT_FRAME_PIPELINE, 1)


# what happens between frame 6 and frame 7 of a running static sequence: (event, settings of the two frames after it)
POST_PASSES = [F.PASS_DEMODULATION, F.PASS_DENOISE_L0, F.PASS_DENOISE_L3, F.PASS_TONE_MAPPING]
EVENTS = {
    "clear_colour": (None, dict(clear_color=(0.1, 0.7, 0.2, 1.0))),
    "denoise_off": (None, dict(denoise=False)),
    "bounces_0": (None, dict(indirect_bounces=0)),
    "resize_and_back": (resize_and_back, {}),
    **{f"pass_run_{k}": ((lambda pair, w, h, k=k: hand_driven(pair, [k])), {}) for k in POST_PASSES},
}


# (a changed setting holds for one frame - one parity's chain - or for two)
EVENT_CASES = [(name, k) for name, (event, _) in EVENTS.items() for k in ((1,) if event else (1, 2))]


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name,changed_frames", EVENT_CASES, ids=[f"{n}-{k}" for n, k in EVENT_CASES])
def test_event_ends_the_grant(pair, size, name, changed_frames):
    """six static frames, the event, six frames after it - one or two of them with the changed settings where the event is a setting,
    then the first settings again: every buffer after every frame"""
    w, h = size
    event, changed = EVENTS[name]
    fresh(pair, w, h)
    for n in range(1, 7):
        frame(pair, "centred", w, h, settings(), n, (name, "before"))
    if event:
        event(pair, w, h)
    for n in range(7, 13):
        frame(pair, "centred", w, h, settings(**changed) if n < 7 + changed_frames else settings(), n, (name, "after"))


def garbage(pair, buf):
    """the same non-constant bytes into one plane of both contexts (0x3c .. 0x3f: finite in f32 and f16, no two neighbouring bytes equal)"""
    for p in pair:
        plane = p.engine.read(buf).copy()
        flat = plane.view(np.uint8).reshape(-1)
        flat[:] = (0x3C + (np.arange(flat.size) % 4)).astype(np.uint8)
        p.engine.write(buf, plane)


POST_PLANES = {**{f"internal{k}": F.BUF_DENOISE_INTERNAL0 + k for k in range(4)}, "internal_variance": F.BUF_DENOISE_INTERNAL_VARIANCE,
               **{f"denoise_render{k}": F.BUF_DENOISE_RENDER0 + k for k in range(3)}, "tone_mapped": F.BUF_TONE_MAPPED,
               "previous_tone_mapped": F.BUF_PREVIOUS_TONE_MAPPED}
# (the reservoir buffers: whichever of the ten is `current` of the indirect channel in the frame after, whose uniform tiles the spatial
# pass's background re-pack reads - and every other one)
RESERVOIRS = {f"reservoir{k}": F.BUF_RESERVOIR0 + k for k in range(10)}


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("name", list(POST_PLANES) + list(RESERVOIRS))
def test_the_next_frames_restore_a_plane_the_host_wrote(pair, size, name):
    w, h = size
    fresh(pair, w, h)
    for n in range(1, 7):
        frame(pair, "centred", w, h, settings(), n, (name, "before"))
    garbage(pair, {**POST_PLANES, **RESERVOIRS}[name])
    for n in range(7, 11):
        frame(pair, "centred", w, h, settings(), n, (name, "after"))
    if name in POST_PLANES:   # (every byte of the plane is the chain's own again, not only equal in both contexts)
        on = pair[0]
        for b in (POST_PLANES[name], F.BUF_TONE_MAPPED, F.BUF_PREVIOUS_TONE_MAPPED):
            words = on.engine.read(b).view(np.uint8).reshape(-1, 4)
            assert not (words == np.array([0x3C, 0x3D, 0x3E, 0x3F], dtype=np.uint8)).all(axis=1).any(), (name, b, "garbage left")
