"""The spatial pass's background (DESIGN 4 "Empty tiles"): a wave of background pixels whose input tile holds one of the two records the
temporal passes store there takes the re-pack of that record, and its id, from a table computed once per context - no load, no unpack, no
pack - and the windowed form of the kernel takes the empty-tile and kept-tile planes as the plain form does.  A context with
HK_DEBUG_OPT_SPATIAL_KNOWN at 0 is handed no table and, in the windowed form, no planes: given the same frames the two must agree in every
byte of every buffer after EVERY frame, in both forms of the kernel, at sizes with partial edge tiles, waves with lanes beyond the image
and a depth window larger than the image."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from cases import diff_buffers, make_case, oracle, snapshot
from test_background_stores_gpu import BASE, camera, fresh, settings

pytestmark = pytest.mark.gpu

SIZES = [(75, 43), (200, 43)]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]
FORMS = {"plain": 0, "windowed": 1}   # HK_DEBUG_OPT_SPATIAL_WINDOW


@pytest.fixture(scope="module")
def pair():
    """(the library's default, HK_DEBUG_OPT_SPATIAL_KNOWN 0): two contexts that are given the same frames throughout"""
    scene = hk.load_cornell()
    on, off = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    off.engine.set_debug_option(F.DEBUG_OPT_SPATIAL_KNOWN, 0)
    for p in (on, off):
        p.set_scene(scene)
    return on, off


def start(pair, w, h, form):
    """a fresh history at this size, the form forced; returns the table launches of both contexts so far"""
    fresh(pair, w, h)
    for p in pair:
        p.engine.set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, FORMS[form])
    return [p.engine.spatial_known_launches() for p in pair]


def compare(pair, what):
    bad = diff_buffers(snapshot(pair[0]), snapshot(pair[1]))
    assert bad == {}, (what, bad)


def frame(pair, view, w, h, s, n, what):
    for p in pair:
        p.render(camera(view, w, h), s, frame_number=n)
    compare(pair, (what, "frame", n, view))


def assert_counts(pair, before, spatial_launches):
    """the switch: every spatial launch of the default context was handed the table, none of the other's"""
    assert pair[0].engine.spatial_known_launches() - before[0] == spatial_launches
    assert pair[1].engine.spatial_known_launches() == before[1] == 0


# (settings, (view, frame number) per frame).  The static view with the indirect pass alone: a channel whose spatial pass is off keeps the
# reference's scatter race once the camera moves (tests/test_known_results_gpu.py), so the sequences that move run both passes - where
# the emissive channel meets the table's second entry.  `pan`: tiles turn empty and non-empty in both frame parities, with tiles that
# are empty in frames n - 2 and n but not in n - 1 (the gap of tests/test_post_stores_gpu.py).
SEQUENCES = {
    "indirect_alone": (dict(emissive_spatial_reuse=False), [("centred", n) for n in range(1, 7)]),
    "both_passes": ({}, [("centred", n) for n in range(1, 7)]),
    "all_background": ({}, [("away", n) for n in range(1, 6)]),
    "pan": ({}, list(zip(["centred", "centred", "centred", "centred", "panned", "centred", "centred", "panned"], range(1, 9)))),
    "no_denoise_b0": (dict(indirect_bounces=0, denoise=False), [("centred", n) for n in range(1, 5)]),
}


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_every_frame_equals_the_long_way(pair, size, form, name):
    w, h = size
    kw, frames = SEQUENCES[name]
    s = settings(**kw)
    before = start(pair, w, h, form)
    windowed = [p.engine.spatial_windowed_launches() for p in pair]
    for view, n in frames:
        frame(pair, view, w, h, s, n, (name, form))
    passes = int(s.emissive_spatial_reuse) + int(s.indirect_spatial_reuse)
    assert_counts(pair, before, passes * len(frames))
    for p, had in zip(pair, windowed):
        assert p.engine.spatial_windowed_launches() - had == (passes * len(frames) if FORMS[form] else 0)
    assert pair[0].engine.empty_tiles()[1] > 0   # (the planes were granted: both forms were handed them)


def background_tiles(engine):
    """[h, w] mask of the pixels that lie in 8x8 tiles (clipped at the image's edge) whose depths are all zero"""
    depth = engine.read(F.BUF_POSITION)[..., 3]
    h, w = depth.shape
    padded = np.zeros(((h + 7) // 8 * 8, (w + 7) // 8 * 8), dtype=bool)
    padded[:h, :w] = depth != 0.0
    empty = ~padded.reshape(padded.shape[0] // 8, 8, padded.shape[1] // 8, 8).any(axis=(1, 3))
    return np.repeat(np.repeat(empty, 8, axis=0), 8, axis=1)[:h, :w]


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("form", list(FORMS))
def test_garbage_in_current_takes_the_long_way(pair, size, form):
    """Six static frames, then the host writes records of its own into the background tiles of the indirect channel's temporal buffer and
    the spatial pass runs again (hk_pass_run).  The tile records are gone with the write: the pass must re-pack what it finds there -
    the short way would store the known record's re-pack instead."""
    w, h = size
    s = settings()
    start(pair, w, h, form)
    for n in range(1, 7):
        frame(pair, "centred", w, h, s, n, ("garbage", "before"))
    prev = 1 - 6 % 2
    current, spatial = F.BUF_RESERVOIR0 + 6 + prev, F.BUF_RESERVOIR0 + 8 + prev   # (context.hip make_light_targets, the indirect channel)
    mask = background_tiles(pair[0].engine)
    assert mask.any() and not mask.all()
    known = pair[0].engine.read(spatial)[mask]
    assert (known == known[0]).all()   # one record in every background tile: the known record's re-pack
    for p in pair:
        plane = p.engine.read(current).copy()
        flat = plane.view(np.uint8).reshape(h, w, -1)
        flat[mask] = (0x3C + (np.arange(flat.shape[2]) % 4)).astype(np.uint8)   # (0x3c .. 0x3f: finite in f32 and f16)
        p.engine.write(current, plane)
        p.engine.pass_run(F.PASS_INDIRECT_SPATIAL_REUSE)
    compare(pair, "the spatial pass over the host's records")
    for p in pair:
        got = p.engine.read(spatial)[mask]
        assert (got == got[0]).all() and (got[0] != known[0]).any(), "the host's records were not re-packed"
    for n in range(7, 10):   # ... and the frames after it restore everything, in both contexts alike
        frame(pair, "centred", w, h, s, n, ("garbage", "after"))


@pytest.mark.parametrize("form", list(FORMS))
def test_ratio_other_than_one_takes_the_table_alone(pair, form):
    """upscale ratio 1.5: no empty-tile plane is granted, the table still applies"""
    w, h = 75, 43
    s15 = hk.HikariSettings(upscale=hk.Upscale.Fsr1(1.5, 0.2), **BASE)
    for p in pair:
        p._size = p._previous_camera = None   # (the first frame resizes for the ratio: a fresh history, no previous view)
        p.engine.set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, FORMS[form])
    before = [p.engine.spatial_known_launches() for p in pair]
    planes = pair[0].engine.empty_tiles()[1]
    for n in range(1, 6):
        for p in pair:
            p.render(camera("centred", w, h), s15, frame_number=n)
        compare(pair, ("ratio 1.5", form, n))
    assert pair[0].engine.empty_tiles()[1] == planes
    assert_counts(pair, before, 2 * 5)


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("split", [24, 21])
def test_spatial_passes_in_two_row_ranges(pair, size, form, split):
    """Four frames, then a frame whose temporal stage runs through hk_frame_stage and whose spatial passes are dispatched by hand in two
    row ranges - cut on a tile row (the tile records are kept: the table applies) and inside one (no tile records: the long way)"""
    w, h = size
    s = settings()
    before = start(pair, w, h, form)
    for n in range(1, 5):
        frame(pair, "centred", w, h, s, n, ("row ranges", "before"))
    cam = camera("centred", w, h)
    for p in pair:
        p.engine.frame_begin(hk.frame_uniform(s, 5), cam.view_uniform(), cam.previous_view_uniform(p._previous_camera), hk.lights_uniform())
        p.engine.frame_stage(F.STAGE_TEMPORAL, s.to_c())
        for pass_id in (F.PASS_EMISSIVE_SPATIAL_REUSE, F.PASS_INDIRECT_SPATIAL_REUSE):
            p.engine.pass_run(pass_id, 0, 0, split)
            p.engine.pass_run(pass_id, 0, split, h)
        p._previous_camera = cam
    compare(pair, ("row ranges", split))
    assert_counts(pair, before, 2 * 4 + 4)
    for n in range(6, 9):
        frame(pair, "centred", w, h, s, n, ("row ranges", "after"))


@pytest.mark.parametrize("form", list(FORMS))
def test_against_the_oracle(form):
    """cornell_b2 of tests/cases.py (96 x 64, mixed tiles, six frames), either form forced: every buffer of every frame, bit for bit"""
    case = make_case("cornell_b2")
    gpu, cpu = hk.HikariPlugin(device=0), oracle()
    gpu.engine.set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, FORMS[form])
    for p in (gpu, cpu):
        p.set_scene(case.scene)
    for n in case.frames:
        for p in (gpu, cpu):
            p.render(case.camera, case.settings, lights=case.lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(cpu))
        assert bad == {}, f"cornell_b2, {form}, frame {n}: {bad}"
    assert gpu.engine.spatial_known_launches() == len(case.frames)
    assert gpu.engine.empty_tiles()[1] > 0
