"""k_spatial_reuse - emissive and indirect, plain and windowed - on the adversarial planes of tests/post_planes.py
(`make_spatial_planes`), bit for bit against the oracle: every byte the pass writes (`spatial`, `variance`, `render`), the sentinel bytes
of everything it must leave alone (`current`, `previous_spatial`, `previous`, the G-buffer planes, the tail of `spatial` beyond the
render size), the two forms against each other on a depth plane in which every texel differs, row ranges that cut a wave tile, a tile
row and a workgroup row, the store elision of all-background tiles, and what the reference's own shader wrote on the planes
(tests/golden/wgsl_spatial_planes_*.npz, tests/tools/wgsl_pin.py --spatial-planes).

tests/test_spatial_planes.py holds the oracle to a float64 restatement of the shader on these planes; through bit equality its bounds
hold for the kernels and are not measured again here.

The settings: every set runs at every shape of SPATIAL_WIDTHS x SPATIAL_HEIGHTS, every ratio and both parities, for both channels
and both forms - 90 dispatches per set, channel and form.  `max_spatial_reuse_count` x `max_reservoir_lifetime` (3 x 3) rotate through
those 90 (`limits_of`): each pair meets every set and channel at ten shape / ratio / parity combinations, each limit at thirty."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F

pytestmark = pytest.mark.gpu

SHAPES = [(w, h) for w in PP.SPATIAL_WIDTHS for h in PP.SPATIAL_HEIGHTS]


@pytest.fixture(scope="module")
def engines():
    from oracle_lib import oracle_plugin

    scene = PP.spatial_scene()
    gpu, cpu = hk.HikariPlugin(device=0), oracle_plugin()
    for p in (gpu, cpu):
        p.set_scene(scene)
    yield gpu.engine, cpu.engine
    gpu.engine.set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, -1)


def limits_of(k):
    return PP.SPATIAL_COUNTS[k % 3], PP.SPATIAL_LIFETIMES[(k // 3) % 3]


def cases():
    k = 0
    for shape in SHAPES:
        for ratio in PP.SPATIAL_RATIOS:
            for parity in (2, 3):
                yield shape, ratio, parity, limits_of(k)
                k += 1


def read_all(e, planes):
    out = {name: e.read(buf) for name, buf in planes.outputs.items()}
    out.update({name: e.read(buf) for name, buf in planes.untouched.items()})
    return out


def diff(a, b):
    """names of the buffers whose bytes differ, with the first differing pixel or record"""
    bad = {}
    for name in a:
        x, y = a[name].view(np.uint8).reshape(-1, a[name].shape[-1] * a[name].itemsize), b[name].view(np.uint8).reshape(-1, a[name].shape[-1] * a[name].itemsize)
        ne = (x != y).any(axis=1)
        if ne.any():
            i = int(np.nonzero(ne)[0][0])
            bad[name] = f"{int(ne.sum())} texels, first #{i}: {a[name].reshape(-1, a[name].shape[-1])[i]} vs {b[name].reshape(-1, a[name].shape[-1])[i]}"
    return bad


def run(e, planes, form=None, rows=None):
    """install, one dispatch (or one per row range, in the order given), read; form: 0 plain, 1 windowed - asserted through the launch counter"""
    PP.install_spatial(e, planes)
    if form is not None:
        e.set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, form)
        before = e.spatial_windowed_launches()
    pieces = rows or [(0, 0)]
    for y0, y1 in pieces:
        e.pass_run(planes.pass_id, 0, y0, y1)
    if form is not None:
        assert e.spatial_windowed_launches() - before == (len(pieces) if form else 0)
    return read_all(e, planes)


@pytest.mark.parametrize("channel", [1, 2], ids=["emissive", "indirect"])
@pytest.mark.parametrize("name", PP.SPATIAL_SETS)
def test_both_forms_equal_the_oracle_in_every_byte(engines, name, channel):
    g, c = engines
    bad = {}
    for shape, ratio, parity, (max_count, max_lifetime) in cases():
        planes = PP.make_spatial_planes(name, 7, shape, ratio, channel, parity, max_count, max_lifetime)
        want = run(c, planes)
        for label, buf in planes.untouched.items():          # (the oracle too leaves these alone: what was written is what is read)
            assert (want[label].view(np.uint8) == planes.buffers[buf].view(np.uint8)).all(), label
        for form in (0, 1):
            d = diff(run(g, planes, form), want)
            if d:
                bad[(shape, ratio, parity, max_count, max_lifetime, "windowed" if form else "plain")] = d
    assert bad == {}


@pytest.mark.parametrize("channel", [1, 2], ids=["emissive", "indirect"])
def test_plain_and_windowed_agree_where_every_depth_differs(engines, channel):
    """the `random` set: a read of the wrong texel changes a decision.  At ratios above 1 the 60 x 60 LDS window covers only part of the
    taps' reach and the rest falls through to the plane; the 70-wide shapes hold a middle workgroup whose window neither border cuts."""
    g, c = engines
    bad = {}
    for height in PP.SPATIAL_HEIGHTS:
        for ratio in PP.SPATIAL_RATIOS:
            for parity in (2, 3):
                for seed in (11, 12):
                    planes = PP.make_spatial_planes("random", seed, (70, height), ratio, channel, parity, 100, 7.0)
                    plain, windowed = run(g, planes, 0), run(g, planes, 1)
                    d = diff(windowed, plain)
                    d.update({"oracle:" + k: v for k, v in diff(plain, run(c, planes)).items()})
                    if d:
                        bad[(height, ratio, parity, seed)] = d
    assert bad == {}


@pytest.mark.parametrize("form", [0, 1], ids=["plain", "windowed"])
@pytest.mark.parametrize("name", ["depths", "background", "random"])
def test_row_ranges_write_the_same_bytes_as_one_dispatch(engines, name, form):
    """cuts at 1, 8, 16, 23 and height - 1 - inside a wave tile, on a tile row, on a workgroup row - issued last piece first.  The tile
    records are kept for whole tiles only (attach_tile_meta)."""
    g, _ = engines
    bad = {}
    for shape in ((70, 45), (49, 45), (17, 17), (70, 17), (8, 45)):
        for channel in (1, 2):
            for ratio, parity in ((1.0, 2), (1.5, 3), (2.0, 2)):
                planes = PP.make_spatial_planes(name, 7, shape, ratio, channel, parity, 100, 7.0)
                whole = run(g, planes, form)
                rows = shape[1]
                cuts = sorted({0, rows} | {y for y in (1, 8, 16, 23, rows - 1) if 0 < y < rows})
                d = diff(run(g, planes, form, rows=list(reversed(list(zip(cuts[:-1], cuts[1:]))))), whole)
                if d:
                    bad[(shape, channel, ratio, parity)] = d
    assert bad == {}


@pytest.mark.parametrize("channel", [1, 2], ids=["emissive", "indirect"])
def test_the_elision_of_all_background_tiles(engines, channel):
    """An all-background G-buffer written by the host, the channel's temporal pass (it stores one record per pixel and notes the tiles
    that hold one record everywhere), then the spatial pass twice: the second finds its output tiles holding the re-pack of exactly
    that record and stores nothing.  Against the oracle, and against a context with HK_DEBUG_OPT_KNOWN_RESULTS at 0.  Then one `current`
    record overwritten from the host: hk_write_buffer declares the tiles unknown, and the next dispatch must re-pack it."""
    g, c = engines
    off = hk.HikariPlugin(device=0)
    off.set_scene(PP.spatial_scene())
    off.engine.set_debug_option(F.DEBUG_OPT_KNOWN_RESULTS, 0)
    trio = (g, c, off.engine)
    temporal = F.PASS_DIRECT_EMISSIVE if channel == 1 else F.PASS_INDIRECT
    for shape, parity in (((70, 45), 2), ((17, 17), 3), ((49, 17), 2)):
        planes = PP.make_spatial_planes("terraces", 7, shape, 1.0, channel, parity, 100, 7.0)
        planes.buffers[F.BUF_POSITION][..., 3] = 0.0
        for e in trio:
            e._post_planes_size = None
            PP.install_spatial(e, planes)
            e.set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, -1) if e is not c else None
            e.pass_run(temporal)
            e.pass_run(planes.pass_id)
            e.pass_run(planes.pass_id)
        names = dict(planes.outputs, current=planes.slots["current"])
        got = [{k: e.read(b) for k, b in names.items()} for e in trio]
        assert diff(got[0], got[1]) == {} and diff(got[2], got[1]) == {}, (shape, parity)
        record = got[1]["current"].copy()
        rw, rh = planes.render_size
        spot = (rh // 2) * rw + rw // 2
        record.reshape(-1, 16)[spot] = PP.pack_records(planes.current).reshape(-1, 16)[spot]
        assert (record.reshape(-1, 16)[spot] != got[1]["current"].reshape(-1, 16)[spot]).any()
        for e in trio:
            e.write(planes.slots["current"], record)
            e.pass_run(planes.pass_id)
        got = [{k: e.read(b) for k, b in names.items()} for e in trio]
        assert diff(got[0], got[1]) == {} and diff(got[2], got[1]) == {}, (shape, parity, "after hk_write_buffer")
        assert (got[0]["spatial"].reshape(-1, 16)[spot, :12] == record.reshape(-1, 16)[spot, :12]).all()


def _fixtures():
    from test_spatial_planes import SPATIAL_PLANES_FIXTURES

    return SPATIAL_PLANES_FIXTURES


@pytest.mark.parametrize("form", [0, 1], ids=["plain", "windowed"])
@pytest.mark.parametrize("case", _fixtures(), ids=lambda c: f"{c[0]}-ch{c[1]}-r{int(c[2] * 10)}-f{c[3]}")
def test_gpu_equals_what_the_reference_shader_wrote_on_the_planes(engines, case, form):
    """the kernels against the outputs of the reference's own spatial_reuse on the planes - no oracle in between"""
    from test_spatial_planes import replay_spatial_planes

    engines[0].set_debug_option(F.DEBUG_OPT_SPATIAL_WINDOW, form)
    assert replay_spatial_planes(engines[0], case) == []
