"""k_direct_lit<false> (sun), k_direct_lit<true> (emissive), k_indirect and the queue-based schedule's k_wf_setup / k_wf_final, with the
scatter resolution behind them (previous_slot, store_previous_spatial, k_resolve_scatter_lite, the parked planes), on the adversarial planes of
tests/post_planes.py (`make_temporal_planes`), bit for bit against the oracle: every byte the pass writes (`current`, `previous_spatial`,
`spatial` for background pixels, `variance`, `render`) and the sentinel bytes of everything it must leave alone (`previous`, the G-buffer
planes, the tails of the record buffers beyond the render grid - where, at ratios above 1, a store to a slot one row past the grid would
land).

The `edge` and `random` sets hold stores whose slot lies past previous_spatial and the parked planes (a previous_uv of exactly 1):
previous_slot (hk_light.hpp) lets none of them land, in any form.  These tests must not run against a library without that guard.

The scatter forms a single context has: the light deterministic form (by default where previous_spatial has a reader - the planes switch
both spatial passes on - and for every channel under HK_CTX_DETERMINISTIC_SCATTER), the reference's race under HK_CTX_RACING_SCATTER
(compared on sets in which no two pixels store to one slot), and the full parked form of a band with a history halo, whose parked planes are
compared with the oracle's before anything resolves them.

tests/test_temporal_planes.py holds the oracle to the reference's own shader on these planes and keeps the store index in range."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F

pytestmark = pytest.mark.gpu

SHAPES = [(w, h) for w in PP.SPATIAL_WIDTHS for h in PP.SPATIAL_HEIGHTS]
CHANNELS = pytest.mark.parametrize("channel", [0, 1, 2], ids=["sun", "emissive", "indirect"])
SCENES = ("open", "roofed")


class Pair:
    """one engine per scene, created on first use"""

    def __init__(self, make):
        self.make, self.engines = make, {}

    def __getitem__(self, scene):
        if scene not in self.engines:
            p = self.make()
            p.set_scene(PP.temporal_scene(scene))
            self.engines[scene] = p
        return self.engines[scene].engine


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import oracle_plugin

    return Pair(oracle_plugin)


@pytest.fixture(scope="module")
def gpu():
    return Pair(lambda: hk.HikariPlugin(device=0))


@pytest.fixture(scope="module")
def gpu_deterministic():
    return Pair(lambda: hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER))


@pytest.fixture(scope="module")
def gpu_racing():
    return Pair(lambda: hk.HikariPlugin(device=0, flags=F.CTX_RACING_SCATTER))


def scene_for(channel, k=0):
    return "roofed" if channel == 1 or k % 2 else "open"


def cases(all_ratios_at=((70, 45),)):
    """every shape once, ratio and parity in turn; the shapes of `all_ratios_at` at every ratio and parity: (k, shape, ratio, parity)"""
    k = 0
    for shape in SHAPES:
        combos = [(r, q) for r in PP.SPATIAL_RATIOS for q in (2, 3)] if shape in all_ratios_at else [(PP.SPATIAL_RATIOS[k % 3], 2 + (k // 3) % 2)]
        for ratio, parity in combos:
            yield k, shape, ratio, parity
            k += 1


def read_all(e, planes):
    out = {name: e.read(buf) for name, buf in planes.outputs.items()}
    out.update({name: e.read(buf) for name, buf in planes.untouched.items()})
    return out


def diff(a, b):
    """names of the buffers whose bytes differ, with the first differing pixel or record"""
    bad = {}
    for name in a:
        width = a[name].shape[-1] * a[name].itemsize
        x, y = a[name].view(np.uint8).reshape(-1, width), b[name].view(np.uint8).reshape(-1, width)
        ne = (x != y).any(axis=1)
        if ne.any():
            i = int(np.nonzero(ne)[0][0])
            bad[name] = f"{int(ne.sum())} texels, first #{i}: {a[name].reshape(-1, a[name].shape[-1])[i]} vs {b[name].reshape(-1, a[name].shape[-1])[i]}"
    return bad


def run(e, planes, rows=None):
    """install, one dispatch (or one per row range, in the order given), read"""
    PP.install_temporal(e, planes)
    for y0, y1 in rows or [(0, 0)]:
        e.pass_run(planes.pass_id, 0, y0, y1)
    return read_all(e, planes)


def oracle_run(oracle, planes):
    want = run(oracle[planes.scene], planes)
    for label, buf in planes.untouched.items():          # (the oracle too leaves these alone: what was written is what is read)
        assert (want[label].view(np.uint8) == planes.buffers[buf].view(np.uint8)).all(), label
    rw, rh = planes.render_size
    for label in ("current", "previous_spatial", "spatial"):   # ... and the record buffers beyond the render grid
        assert (want[label].reshape(-1, 16)[rw * rh:] == PP.SENTINEL_U32).all(), label
    return want


# ---------------------------------------------------------------- every byte, every set, every channel, both scenes
@CHANNELS
@pytest.mark.parametrize("name", PP.TEMPORAL_SETS)
def test_every_byte_equals_the_oracle(gpu, oracle, name, channel):
    bad = {}
    scenes = set()
    for k, shape, ratio, parity in cases():
        planes = PP.make_temporal_planes(name, 7, shape, ratio, channel, parity, scene=scene_for(channel, k))
        scenes.add(planes.scene)
        d = diff(run(gpu[planes.scene], planes), oracle_run(oracle, planes))
        if d:
            bad[(shape, ratio, parity, planes.scene)] = d
    assert bad == {}
    assert scenes == ({"roofed"} if channel == 1 else set(SCENES))


@CHANNELS
@pytest.mark.parametrize("name", ["thresholds", "records"])
def test_the_settings_the_decisions_read(gpu, oracle, name, channel):
    """validate intervals 1 and the defaults on validation and other frame numbers, max_temporal_reuse_count 1, 4 and 65504 (the `clamp`
    pixels carry counts of the limit -1, +0, +1), temporal_reuse off, at the shapes that hold a partial tile and two workgroups"""
    bad = {}
    settings = [dict(direct_validate_interval=1, emissive_validate_interval=1, max_temporal_reuse_count=1), dict(max_temporal_reuse_count=4),
                dict(max_temporal_reuse_count=65504), dict(temporal_reuse=False), dict(direct_validate_interval=1, emissive_validate_interval=1, temporal_reuse=False)]
    k = 0
    for shape in ((17, 17), (70, 45)):
        for frame_number in (2, 3, 5, 15):                         # 3 and 15 validate the sun, 5 and 15 the emitters (the defaults: 3 and 5)
            for extra in settings:
                planes = PP.make_temporal_planes(name, 7, shape, PP.SPATIAL_RATIOS[k % 3], channel, frame_number, scene=scene_for(channel, k), **extra)
                k += 1
                d = diff(run(gpu[planes.scene], planes), oracle_run(oracle, planes))
                if d:
                    bad[(shape, frame_number, tuple(extra.items()))] = d
    assert bad == {}


# ---------------------------------------------------------------- the scatter forms
@CHANNELS
@pytest.mark.parametrize("name", ["scatter", "edge", "random"])
def test_the_deterministic_forms_agree_on_contested_slots(gpu, gpu_deterministic, oracle, name, channel):
    """HK_CTX_DETERMINISTIC_SCATTER and the default (both the light form: parked where the slot is another pixel's, resolved by
    k_resolve_scatter_lite) against the oracle's highest index wins - and with the spatial passes off, where the default races, the
    flag alone must still resolve"""
    bad = {}
    for k, shape, ratio, parity in cases(all_ratios_at=()):
        for seed in ((7, 8) if name == "random" else (7,)):
            planes = PP.make_temporal_planes(name, seed, shape, ratio, channel, parity, scene=scene_for(channel, k))
            want = oracle_run(oracle, planes)
            for label, engines in (("default", gpu), ("deterministic", gpu_deterministic)):
                d = diff(run(engines[planes.scene], planes), want)
                if d:
                    bad[(shape, ratio, parity, seed, label)] = d
    for shape in ((70, 45), (49, 17)):
        planes = PP.make_temporal_planes(name, 7, shape, 1.5, channel, 2, scene=scene_for(channel), emissive_spatial_reuse=False, indirect_spatial_reuse=False)
        d = diff(run(gpu_deterministic[planes.scene], planes), oracle_run(oracle, planes))
        if d:
            bad[(shape, "no reader", "deterministic")] = d
    assert bad == {}


@CHANNELS
@pytest.mark.parametrize("name", ["benign", "thresholds", "records", "background"])
def test_the_race_where_nothing_is_contested(gpu_racing, oracle, name, channel):
    """HK_CTX_RACING_SCATTER on the sets in which every pixel stores to its own slot at most: the reference's own stores, no parking"""
    bad = {}
    for k, shape, ratio, parity in cases(all_ratios_at=()):
        planes = PP.make_temporal_planes(name, 7, shape, ratio, channel, parity, scene=scene_for(channel, k))
        assert PP.temporal_store_targets(planes)[1]["to_other_slot"] == 0
        d = diff(run(gpu_racing[planes.scene], planes), oracle_run(oracle, planes))
        if d:
            bad[(shape, ratio, parity)] = d
    assert bad == {}


@CHANNELS
def test_a_band_parks_what_the_oracle_parks_and_nothing_for_a_discarded_store(oracle, channel):
    """the full parked form (a band of a sharded frame with a history halo): every store waits in the parked planes - the slot per pixel,
    -1 where a pixel stores nothing or its slot lies past the grid, and the record - until stage SPATIAL.  Plane for plane against the
    oracle's park_scatter, before anything resolves."""
    from oracle_lib import oracle_plugin

    bad = {}
    for scene in ("roofed",) if channel == 1 else SCENES:
        g, c = hk.HikariPlugin(device=0), oracle_plugin()
        for p in (g, c):
            p.set_scene(PP.temporal_scene(scene))
            p.engine.set_band(0, 2)
            p.engine.set_history_rows(4)
        for name, shape, ratio, parity in (("edge", (17, 17), 1.0, 2), ("edge", (70, 45), 1.5, 3), ("scatter", (70, 45), 1.0, 2), ("random", (49, 45), 2.0, 3)):
            planes = PP.make_temporal_planes(name, 7, shape, ratio, channel, parity, scene=scene)
            rw, rh = planes.render_size
            got = []
            for p in (g, c):
                PP.install_temporal(p.engine, planes)
                p.engine.pass_run(planes.pass_id)
                to = p.engine.read(F.BUF_PARKED_TO0 + channel).view(np.int32).reshape(-1)[:rw * rh]
                record = p.engine.read(F.BUF_PARKED_RECORD0 + channel).reshape(-1, 16)[:rw * rh]
                got.append((to, record, {k: p.engine.read(b) for k, b in planes.outputs.items() if k != "previous_spatial"}))
            (to_g, rec_g, out_g), (to_c, rec_c, out_c) = got
            index, counts, _ = PP.temporal_store_targets(planes)
            if name != "scatter":
                assert counts["discarded"] >= 1
            assert ((to_c >= -1) & (to_c < rw * rh)).all()
            if not (to_g == to_c).all():
                bad[(scene, name, shape, "slot")] = int((to_g != to_c).sum())
            parked = to_c >= 0
            if not (rec_g[parked] == rec_c[parked]).all():
                bad[(scene, name, shape, "record")] = int((rec_g[parked] != rec_c[parked]).any(axis=1).sum())
            d = diff(out_g, out_c)
            if d:
                bad[(scene, name, shape, "outputs")] = d
    assert bad == {}


# ---------------------------------------------------------------- the schedules of indirect_lit_ambient
@pytest.mark.parametrize("bounces", [1, 2])
def test_the_fused_and_the_queue_based_indirect_pass_write_the_same_bytes(oracle, bounces):
    """k_indirect against k_wf_setup / k_wf_final (both run indirect_temporal_tail) and the oracle, on the roofed scene where bounces hit.
    The queue-based schedule exists from two bounces on: at one bounce both contexts run k_indirect, its single-bounce instantiation."""
    fused, wavefront = Pair(lambda: hk.HikariPlugin(device=0, flags=F.CTX_FUSED_INDIRECT)), Pair(lambda: hk.HikariPlugin(device=0, flags=F.CTX_WAVEFRONT))
    bad = {}
    k = 0
    for name in ("edge", "scatter", "thresholds", "random"):
        for shape in ((70, 45), (17, 17), (49, 1), (1, 45)):
            planes = PP.make_temporal_planes(name, 7, shape, PP.SPATIAL_RATIOS[k % 3], 2, 2 + k % 2, scene="roofed" if k % 4 else "open", indirect_bounces=bounces)
            k += 1
            a, b = run(fused[planes.scene], planes), run(wavefront[planes.scene], planes)
            assert fused[planes.scene].indirect_schedule() == "fused" and wavefront[planes.scene].indirect_schedule() == ("wavefront" if bounces >= 2 else "fused")
            d = diff(a, b)
            d.update({"oracle:" + key: v for key, v in diff(a, oracle_run(oracle, planes)).items()})
            if d:
                bad[(name, shape, planes.ratio, planes.scene)] = d
    assert bad == {}


# ---------------------------------------------------------------- the walks
@CHANNELS
def test_the_product_default_walks_write_the_same_bytes(oracle, channel):
    """product_default_plugin(): no exact-traversal flag - these scenes fit the LDS copy and are walked one level, from LDS"""
    from cases import product_default_plugin

    default = Pair(product_default_plugin)
    bad = {}
    k = 0
    for name in ("benign", "edge", "scatter", "random"):
        for shape in ((70, 45), (17, 17), (8, 1)):
            planes = PP.make_temporal_planes(name, 7, shape, PP.SPATIAL_RATIOS[k % 3], channel, 2 + k % 2, scene=scene_for(channel, k + 1))
            k += 1
            d = diff(run(default[planes.scene], planes), oracle_run(oracle, planes))
            if d:
                bad[(name, shape, planes.ratio, planes.scene)] = d
    assert bad == {}


# ---------------------------------------------------------------- row ranges
@CHANNELS
@pytest.mark.parametrize("form", ["default", "deterministic"])
@pytest.mark.parametrize("name", ["scatter", "edge", "random"])
def test_row_ranges_write_the_same_bytes_as_one_dispatch(gpu, gpu_deterministic, name, form, channel):
    """cuts at 1, 8, 16, 23 and height - 1 - inside a wave tile, on a tile row, on a workgroup row - issued last piece first, in order and
    interleaved; the scatter set stores from one piece into another's slots, in both directions.  (A piece takes the full parked form and
    resolves over the whole image: the light form decided per piece and the bytes depended on the order - context.hip run_pass.)"""
    bad = {}
    for shape in ((70, 45), (49, 45), (17, 17), (8, 45)):
        for ratio, parity in ((1.0, 2), (1.5, 3)):
            planes = PP.make_temporal_planes(name, 7, shape, ratio, channel, parity, scene=scene_for(channel))
            e = (gpu if form == "default" else gpu_deterministic)[planes.scene]
            whole = run(e, planes)
            rows = shape[1]
            cuts = sorted({0, rows} | {y for y in (1, 8, 16, 23, rows - 1) if 0 < y < rows})
            pieces = list(zip(cuts[:-1], cuts[1:]))
            for label, order in (("last first", pieces[::-1]), ("in order", pieces), ("odd ones first", pieces[1::2] + pieces[::2])):
                d = diff(run(e, planes, rows=order), whole)
                if d:
                    bad[(shape, ratio, parity, label)] = d
    assert bad == {}


# ---------------------------------------------------------------- the uniform-tile elision
@CHANNELS
def test_the_elision_of_all_background_tiles_and_its_poison(gpu, oracle, channel):
    """`background` twice: the second dispatch finds its all-background tiles holding the record already and stores nothing there -
    against the oracle and against a context with HK_DEBUG_OPT_KNOWN_RESULTS at 0.  Then the racing form scatters a store into such a
    tile (a geometry pixel aimed at a background pixel's slot): the tile's poison makes the next dispatch store the background record again."""
    scene = scene_for(channel)
    off = hk.HikariPlugin(device=0)
    off.set_scene(PP.temporal_scene(scene))
    off.engine.set_debug_option(F.DEBUG_OPT_KNOWN_RESULTS, 0)
    racing = hk.HikariPlugin(device=0, flags=F.CTX_RACING_SCATTER)
    racing.set_scene(PP.temporal_scene(scene))
    for shape, ratio, parity in (((70, 45), 1.0, 2), ((49, 17), 1.5, 3), ((70, 17), 2.0, 2)):
        planes = PP.make_temporal_planes("background", 7, shape, ratio, channel, parity, scene=scene)
        rw, rh = planes.render_size
        trio = (gpu[scene], oracle[scene], off.engine, racing.engine)
        for e in trio:
            e._post_planes_size = None
            PP.install_temporal(e, planes)
            e.pass_run(planes.pass_id)
            e.pass_run(planes.pass_id)
        got = [read_all(e, planes) for e in trio]
        for other in (0, 2, 3):
            assert diff(got[other], got[1]) == {}, (shape, ratio, other)
        # a geometry pixel (the corner lane of tile (4, 0): render pixel (32, 0)) looks at background pixel (3, 2), inside an all-background
        # tile that the dispatches above left elided; its history fails, so it stores a zero record there:
        # the owner, a background pixel with a LOWER index, loses to it (highest index wins)
        source, target = (32, 0), (3, 0)
        tx, ty = PP.spatial_texel(planes, *source)
        ju, jv = PP.temporal_jittered_uv(planes, *source)
        velocity = planes.buffers[F.BUF_VELOCITY_UV].copy()
        velocity[ty, tx, 0] = np.float32(ju - np.float32(np.float32(target[0] + 0.5) / np.float32(rw)))
        velocity[ty, tx, 1] = np.float32(jv - np.float32(np.float32(target[1] + 0.5) / np.float32(rh)))
        assert PP.temporal_target(planes, *source, velocity[ty, tx, :2])[3] == target[0] + rw * target[1]
        for e in trio:
            e.write(F.BUF_VELOCITY_UV, velocity)
            e.pass_run(planes.pass_id)
        got = [{k: e.read(b) for k, b in planes.outputs.items()} for e in trio]
        for other in (0, 2, 3):
            assert diff(got[other], got[1]) == {}, (shape, ratio, other, "scattered into an elided tile")
        slot = target[0] + rw * target[1]
        background_record = got[1]["previous_spatial"].reshape(-1, 16)[slot + 1]
        # (direct light: a background pixel's record has count 1, the refused history that lands is the empty record.  indirect_lit_ambient
        # stores the empty record for both: there the poison cannot show in the bytes, only the equalities above hold it)
        assert channel == 2 or (got[1]["previous_spatial"].reshape(-1, 16)[slot] != background_record).any(), "the scattered store must have landed"
        # the velocity back: the next dispatch must put the background record back into the poisoned tile
        for e in trio:
            e.write(F.BUF_VELOCITY_UV, planes.buffers[F.BUF_VELOCITY_UV])
            e.pass_run(planes.pass_id)
        got = [{k: e.read(b) for k, b in planes.outputs.items()} for e in trio]
        for other in (0, 2, 3):
            assert diff(got[other], got[1]) == {}, (shape, ratio, other, "after the poison")
        assert (got[0]["previous_spatial"].reshape(-1, 16)[slot] == background_record).all()


# ---------------------------------------------------------------- what the reference's own shader wrote
def _fixtures():
    from test_temporal_planes import TEMPORAL_PLANES_FIXTURES

    return TEMPORAL_PLANES_FIXTURES


@pytest.mark.parametrize("form", ["default", "deterministic"])
@pytest.mark.parametrize("case", _fixtures(), ids=lambda c: f"{c[0]}-ch{c[1]}-r{int(c[2] * 10)}-f{c[3]}-{c[4]}")
def test_gpu_equals_what_the_reference_shader_wrote_on_the_planes(gpu, gpu_deterministic, case, form):
    """the kernels against the outputs of the reference's own direct_lit / indirect_lit_ambient on the planes - no oracle in between"""
    from test_temporal_planes import replay_temporal_planes

    assert replay_temporal_planes(gpu if form == "default" else gpu_deterministic, case) == []
