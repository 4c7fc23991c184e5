"""The oracle's temporal light passes - direct_lit for the sun and for emitters, indirect_lit_ambient (light.wgsl:917-952, 1040-1240,
1452-1497) - on the adversarial planes of tests/post_planes.py (`make_temporal_planes`): a host-written G-buffer and a host-built
`previous` reservoir buffer that put operands ON the decisions of reprojection, check_previous_reservoir, the validation frame, the
clamp and the scattered store into another pixel's slot of previous_spatial.

Held here, without a GPU:

  the store index   light.wgsl loads history where |uv - 0.5| < 0.5 and stores where it is <= 0.5: a previous_uv.y of exactly 1, or an x of
                    exactly 1 on the last row, forms a slot one row PAST previous_spatial.  `temporal_store_targets` replays the index
                    arithmetic in f32 (it is exact there); every slot it forms is in range or counted as discarded, `edge` discards at
                    least one store per channel in every shape, and the oracle leaves every byte beyond the render grid alone.
  the sets          each set reaches what it was built for (`TemporalPlanes.branches`, non-zero per purpose), and every edge value of
                    previous_uv is the f32 the velocity was built to yield.
  a host sanitizer  tests/native/temporal_oracle_main.cpp links oracle/hk_oracle.cpp alone and replays one `edge` dispatch per channel from
                    a flat dump of the planes, built with -fsanitize=address,undefined.  Nothing is loaded into Python for it.
  the shader        tests/golden/wgsl_temporal_planes_*.npz hold what the reference's own light.wgsl wrote on `edge`, `thresholds`,
                    `scatter` and `records` planes (tests/tools/wgsl_pin.py --temporal-planes), scatter resolved by highest invocation
                    index, stores beyond the array dropped; the oracle must write the same bytes.

tests/test_temporal_planes_gpu.py holds the kernels to the oracle and to the fixtures bit for bit, in every scatter form.

  float64           tests/temporal_restated.py restates all three passes from the shader's text on the open scene, where each new sample is
                    analytic - an unoccluded sun, no emissive candidate, a bounce ray that misses into the ambient term - with per-pixel
                    outcomes (history taken; refused by depth, normal, instance alone; outside; sample merged / picked; clamp hit;
                    validation traced / replaced / kept; store scattered / discarded / to the own slot; background) and a `margin` mask by
                    reason.  The oracle is bounded against it on `benign`, per channel, over every shape, ratio and frames 2, 3 and 5.
                    Measured worst deviation (render, statistics in f16 ulps; variance in f32 ulps of the minuend) and BOUNDS = twice that,
                    next whole ulp:   sun 4.425 / 0.5001 / 2.563 -> 9 / 2 / 6;   emissive 6.847 / 0.5001 / 8.593 -> 14 / 2 / 18;
                    indirect 3.970 / 9.661 / 2955.9 -> 8 / 20 / 5912.  At most 2 % of the geometry pixels (one whole pixel in small shapes)
                    may be `margin`, none `open`; measured: at most two pixels of a dispatch.  The eight planted mistakes must fail on every
                    channel on which they can show (NOT_APPLICABLE says which cannot and why, and that claim is asserted).  Each set must
                    TAKE the branches it was built for, per channel, by these outcomes; the slot index property is taken from the
                    restatement, per channel.  Not restated: two and more bounces (nothing is hit on the open scene: the loop ends at the
                    first miss), and everything on the roofed scene - the shader fixtures and bit equality hold those."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import post_planes as PP
from bevy_hikari_amd import _ffi as F

SHAPES = [(w, h) for w in PP.SPATIAL_WIDTHS for h in PP.SPATIAL_HEIGHTS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shader_fixture_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import wgsl_pin

    return wgsl_pin


def scene_for(channel, k=0):
    """the emissive pass samples nothing in a scene without emitters: it gets the roofed scene; the others alternate"""
    return "roofed" if channel == 1 or k % 2 else "open"


@pytest.fixture(scope="module")
def oracles():
    from oracle_lib import oracle_plugin

    out = {}
    for kind in ("open", "roofed"):
        p = oracle_plugin()
        p.set_scene(PP.temporal_scene(kind))
        out[kind] = p.engine
    return out


# ---------------------------------------------------------------- the planes themselves
def test_velocity_for_hits_the_value_it_names_or_says_it_cannot():
    one = np.float32(1.0)
    want = {"zero": 0.0, "under_one": np.nextafter(one, np.float32(0)), "one": one, "over_one": np.nextafter(one, np.float32(2)), "negative": np.float32(-0.25),
            "huge": np.float32(1e9), "half": np.float32(0.5)}
    hit = {k: 0 for k in PP.EDGE_UVS}
    for n in sorted(set(PP.SPATIAL_WIDTHS) | set(PP.SPATIAL_HEIGHTS)):
        for i in range(n):
            j = np.float32(np.float32(i + 0.5) / np.float32(n))
            for kind in PP.EDGE_UVS:
                v, got = PP.velocity_for(j, kind)
                if v is None:
                    continue
                hit[kind] += 1
                with np.errstate(all="ignore"):
                    assert np.float32(j - v).tobytes() == np.float32(got).tobytes()
                if kind in want:
                    assert got == np.float32(want[kind]) and (kind == "negative" or not np.signbit(got))
                elif kind == "nan":
                    assert np.isnan(got)
                else:
                    assert np.isinf(got) and (got > 0) == (kind == "inf")
    assert all(hit.values()), hit
    # exactly 1 is reachable from every pixel centre the shapes hold: the forced corner cases of `edge` never fall through to another value
    for n in sorted(set(PP.SPATIAL_WIDTHS) | set(PP.SPATIAL_HEIGHTS)):
        for i in (0, n - 1):
            assert PP.velocity_for(np.float32(np.float32(i + 0.5) / np.float32(n)), "one")[0] is not None


def test_i32_of_one_times_the_size_is_the_size():
    """what makes the slot past the buffer: i32(1.0 * rh) == rh, so a uv.y of exactly 1 addresses row rh"""
    for n in sorted(set(PP.SPATIAL_WIDTHS) | set(PP.SPATIAL_HEIGHTS)):
        assert int(np.float32(np.float32(1.0) * np.float32(n))) == n
        assert int(np.float32(np.nextafter(np.float32(1.0), np.float32(0.0)) * np.float32(n))) == n - 1


def test_edge_places_every_value_of_previous_uv():
    """what the builder placed (what the pass DECIDES on each set: test_every_set_takes_the_branches_it_was_built_for)"""
    for ratio in PP.SPATIAL_RATIOS:
        for parity in (2, 3):
            p = PP.make_temporal_planes("edge", 7, (70, 45), ratio, 0, parity)
            missing = [k for k in ["uv_" + k for k in PP.EDGE_UVS] + ["store_without_load", "store_discarded", "store_wrapped_in_range"] if not p.branches.get(k)]
            assert missing == [] and p.placed.any(), (ratio, parity, missing)


def test_the_depth_threshold_pixels_sit_one_ulp_either_side():
    """`thresholds`: replay check_previous_reservoir's depth test in f32 on the placed depth pixels - both outcomes occur, in both
    directions of the ratio, and moving the history depth by one ulp towards the current depth flips a refusal"""
    outcomes = set()
    for parity in (2, 3):
        p = PP.make_temporal_planes("thresholds", 7, (70, 45), 1.5, 0, parity)
        f = np.float32
        assert len(p.where["depth"]) >= 8
        for x, y in p.where["depth"]:
            tx, ty = PP.spatial_texel(p, x, y)
            d_cur, d_hist = p.buffers[F.BUF_POSITION][ty, tx, 3], p.previous.visible_position[y, x, 3]
            assert d_cur == np.float32(2.0) and d_hist != d_cur
            thr = f(f(1.05) * f(f(1.0) + f(f(0.5) * PP.temporal_random_x(p, x, y))))
            ratio = lambda d: (lambda q: f(f(1.0) / q) if q < 1 else q)(f(d / d_cur))
            miss = bool(ratio(d_hist) > thr)
            outcomes.add((miss, bool(d_hist > d_cur)))
            if miss:
                assert not ratio(np.nextafter(d_hist, d_cur)) > thr, (x, y)
            else:
                assert ratio(np.nextafter(d_hist, f(np.inf) if d_hist > d_cur else f(0))) > thr, (x, y)
    assert outcomes == {(True, True), (True, False), (False, True), (False, False)}


# ---------------------------------------------------------------- the store past the buffer
@pytest.mark.parametrize("channel", [0, 1, 2], ids=["sun", "emissive", "indirect"])
def test_edge_discards_a_store_and_the_oracle_writes_nothing_beyond_the_render_grid(oracles, channel):
    """`edge` on every shape: at least one store per channel goes to a slot >= rw * rh.  At ratios above 1 the reservoir buffers are
    window-sized, so that slot EXISTS behind the render grid: its sentinel must survive, in previous_spatial and in every other buffer."""
    for k, shape in enumerate(SHAPES):
        ratio = PP.SPATIAL_RATIOS[k % 3]
        p = PP.make_temporal_planes("edge", 7, shape, ratio, channel, 2 + k % 2, scene=scene_for(channel, k))
        rw, rh = p.render_size
        index, counts, unloaded = PP.temporal_store_targets(p)
        assert counts["discarded"] >= 1
        e = oracles[p.scene]
        PP.install_temporal(e, p)
        e.pass_run(p.pass_id)
        for label, buf in p.outputs.items():
            got = e.read(buf)
            if got.shape[-1] == 16:
                tail = got.reshape(-1, 16)[rw * rh:]
                assert (tail == PP.SENTINEL_U32).all(), (shape, ratio, label)
        for label, buf in p.untouched.items():
            assert (e.read(buf).view(np.uint8) == p.buffers[buf].view(np.uint8)).all(), (shape, label)
        # and what an in-range wrap does: the store of a pixel whose uv.x is exactly 1 lands in column 0 of the next row, unless that
        # slot's own pixel (a higher index) stored too - previous_spatial there is no sentinel any more
        ps = e.read(p.slots["previous_spatial"]).reshape(-1, 16)
        wrapped = [int(i) for i in index[unloaded & (index < rw * rh)].ravel()]
        assert len(wrapped) == counts["wrapped_in_range"] and all((ps[i] != PP.SENTINEL_U32).any() for i in wrapped), shape


def test_a_discarded_store_parks_nothing_in_the_banded_form():
    """the cross-band parked form of the oracle (park_scatter): two bands with a history halo; a pixel whose store is discarded leaves
    -1 in the parked-slot plane, and every parked slot is inside the grid"""
    from oracle_lib import oracle_plugin

    p = PP.make_temporal_planes("edge", 7, (17, 17), 1.0, 2, 2)
    rw, rh = p.render_size
    index, counts, unloaded = PP.temporal_store_targets(p)
    assert counts["discarded"] >= 1
    plug = oracle_plugin()
    plug.set_scene(PP.temporal_scene("open"))
    e = plug.engine
    PP.install_temporal(e, p)
    e.set_band(0, 2)
    e.set_history_rows(4)
    e.pass_run(p.pass_id)
    to = e.read(F.BUF_PARKED_TO0 + 2).view(np.int32).reshape(-1)[:rw * rh]
    assert ((to >= -1) & (to < rw * rh)).all()
    assert (to >= 0).any()
    assert (to[(index >= rw * rh).ravel()] == -1).all()
    # ... while a store that wraps in range is parked with its slot
    wrapped = (unloaded & (index < rw * rh)).ravel()
    assert wrapped.any() and (to[wrapped] == index.ravel()[wrapped]).all()


# ---------------------------------------------------------------- the oracle under a host sanitizer: a stand-alone program
def test_oracle_runs_edge_planes_clean_under_address_and_undefined_sanitizers(tmp_path):
    """Against the oracle before the guard this program reports, on the very first dispatch: `runtime error: signed integer overflow:
    2147483647 * 17 cannot be represented in type 'int'` (previous_index formed off screen), and with that alone mended
    `AddressSanitizer: heap-buffer-overflow ... READ of size 1 ... in apply_scatter ... 6 bytes to the right of 289-byte region` - slot
    17 * 17 + 5 of own_written, from a previous_uv.y of exactly 1."""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the oracle itself: it is part of what the suite needs"
    prog = str(tmp_path / "temporal_oracle")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-mfma", "-msse4.1", "-fno-math-errno",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"), "-o", prog, os.path.join(ROOT, "tests", "native", "temporal_oracle_main.cpp"), os.path.join(ROOT, "oracle", "hk_oracle.cpp")]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]
    probed = subprocess.run([gxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    assert probed.returncode == 0, "g++ cannot link the address / undefined sanitizer runtimes (libasan, libubsan): " + probed.stderr[-1000:]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    dumps = []
    for channel in (0, 1, 2):
        p = PP.make_temporal_planes("edge", 7, (17, 17), 1.0 if channel != 1 else 1.5, channel, 2 + channel % 2, scene=scene_for(channel))
        assert PP.temporal_store_targets(p)[1]["discarded"] >= 1
        dumps.append(str(tmp_path / f"edge_ch{channel}.bin"))
        PP.dump_temporal_planes(p, dumps[-1])
    run = subprocess.run([prog] + dumps, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr[-4000:]


# ---------------------------------------------------------------- what the reference's own shader wrote
def replay_temporal_planes(engines, case):
    """tests/golden/wgsl_temporal_planes_<case>.npz holds what the REFERENCE'S SHADER - direct_lit of light.wgsl with RENDER_EMISSIVE or
    EMISSIVE_LIT, indirect_lit_ambient - wrote on the planes of `case` at 24 x 16: `current`, `previous_spatial`, `spatial` (the records the
    pass indexes), `variance`, `render` (tests/tools/wgsl_pin.py --temporal-planes --write, run where the reference is at hand).  Run the
    engine of engines[scene] on the same planes and return the buffers whose bytes differ from what the shader wrote."""
    wgsl_pin = shader_fixture_cases()
    name, channel, ratio, frame_number, scene = case
    data = np.load(wgsl_pin.temporal_planes_fixture_path(*case))
    planes = PP.make_temporal_planes(name, 7, (24, 16), ratio, channel, frame_number, scene=scene)
    e = engines[scene]
    PP.install_temporal(e, planes)
    e.pass_run(planes.pass_id)
    assert {int(k.split("buf")[1]) for k in data.files} == set(planes.outputs.values())
    bad = []
    for key in data.files:
        got = e.read(int(key.split("buf")[1])).view(np.uint8).reshape(-1)
        differs = got[:data[key].size] != data[key]
        if differs.any():
            bad.append((key, int(differs.sum())))
    return bad


TEMPORAL_PLANES_FIXTURES = shader_fixture_cases().TEMPORAL_PLANES_FIXTURES
_ids = lambda c: f"{c[0]}-ch{c[1]}-r{int(c[2] * 10)}-f{c[3]}-{c[4]}"


def test_the_fixtures_cover_what_they_are_for():
    cases = TEMPORAL_PLANES_FIXTURES
    for name in ("edge", "thresholds", "scatter"):
        assert {c[1] for c in cases if c[0] == name} == {0, 1, 2}
    assert {c[1] for c in cases if c[4] == "roofed"} == {0, 1, 2} and {c[2] for c in cases} == {1.0, 1.5} and {c[3] % 2 for c in cases} == {0, 1}
    for case in cases:
        size = os.path.getsize(shader_fixture_cases().temporal_planes_fixture_path(*case))
        assert 8_000 < size < 40_000, (case, size)
    # the edge fixtures hold a discarded store and an in-range wrap; the scatter ones a contested slot
    for case in cases:
        p = PP.make_temporal_planes(case[0], 7, (24, 16), case[2], case[1], case[3], scene=case[4])
        if case[0] == "edge":
            counts = PP.temporal_store_targets(p)[1]
            assert counts["discarded"] >= 1 and counts["wrapped_in_range"] >= 1
        if case[0] == "scatter":
            assert p.branches.get("contested", 0) > 8 and p.branches.get("owner_background")


@pytest.mark.parametrize("case", TEMPORAL_PLANES_FIXTURES, ids=_ids)
def test_oracle_equals_what_the_reference_shader_wrote_on_the_planes(oracles, case):
    assert replay_temporal_planes(oracles, case) == []


@pytest.mark.skipif(not shader_fixture_cases().reference_available(), reason="no reference checkout (HIKARI_REFERENCE_DIR)")
@pytest.mark.parametrize("case", TEMPORAL_PLANES_FIXTURES, ids=_ids)
def test_reference_shader_reproduces_the_oracle_on_the_planes(case):
    """direct_lit / indirect_lit_ambient of light.wgsl itself, executed on the oracle's state: byte for byte, and the committed fixture is
    what it writes"""
    wgsl_pin = shader_fixture_cases()
    results = wgsl_pin.run_temporal_planes(*case)
    assert results and [r for r in results if r["mismatch"]] == []
    data = np.load(wgsl_pin.temporal_planes_fixture_path(*case))
    assert sorted(data.files) == sorted(wgsl_pin.run_temporal_planes.recorded)
    assert all((data[k] == wgsl_pin.run_temporal_planes.recorded[k]).all() for k in data.files)


# ---------------------------------------------------------------- direct_lit for the sun in float64, from light.wgsl (tests/temporal_restated.py)
from temporal_restated import MISTAKES, restate  # noqa: E402
from test_post_chain_planes import deviation_f16  # noqa: E402
from test_spatial_planes import f32_ulp  # noqa: E402


def check(e, planes, mistake=None):
    """one sun dispatch on the oracle against the restatement: ({quantity: worst deviation}, left-out share of the geometry pixels, the
    restatement, problems)"""
    PP.install_temporal(e, planes)
    e.pass_run(planes.pass_id)
    rw, rh = planes.render_size
    grid = lambda name: e.read(planes.outputs[name]).reshape(-1, 16)[:rw * rh].reshape(rh, rw, 16)
    current, previous_spatial = grid("current"), grid("previous_spatial")
    variance, render = e.read(planes.outputs["variance"])[..., 0], e.read(planes.outputs["render"])
    r = restate(planes, mistake)
    skip = r.margin | r.open | r.background
    problems, worst = [], {}
    halves = lambda rec, word: np.stack([(rec[..., word] & 0xFFFF).astype(np.uint16), (rec[..., word] >> 16).astype(np.uint16)], axis=-1)
    first = lambda mask: tuple(int(v) for v in np.argwhere(mask)[0][::-1])
    worst["render"], bad = deviation_f16(r.render, render, skip)
    if bad.any():
        problems.append(f"render: special values disagree at {int(bad.sum())} pixels, first {first(bad)}")
    got_stats = np.concatenate([halves(current, 14), halves(current, 15)], axis=-1)                       # count, w, w_sum, w2_sum
    worst["statistics"], bad = deviation_f16(np.stack([r.count, r.w, r.w_sum, r.w2_sum], axis=-1), got_stats, skip)
    if bad.any():
        problems.append(f"statistics: special values disagree at {int(bad.sum())} pixels, first {first(bad)}")
    got_radiance = np.concatenate([halves(current, 0), halves(current, 1)], axis=-1)
    for label, differs in (("the radiance picked", (got_radiance != r.radiance_bits).any(axis=-1)),
                           ("the stored visible position", (current[..., 4:8] != r.visible_position.view(np.uint32)).any(axis=-1)),
                           ("the lifetime", ((current[..., 12] >> 24).astype(np.int64) != ((r.lifetime - 127.0).astype(np.int64) & 0xFF)))):
        differs = differs & ~skip
        if differs.any():
            problems.append(f"{label} disagrees at {int(differs.sum())} pixels, first {first(differs)}")
    with np.errstate(all="ignore"):
        capped = r.variance >= 10.0 - 1e-6
        dev = np.where(~skip & ~capped & np.isfinite(r.variance), np.abs(variance.astype(np.float64) - r.variance) / f32_ulp(r.variance_unit), 0.0)
        wrong_cap = ~skip & (r.variance >= 10.0 + 1e-5) & (variance != np.float32(10.0))
    worst["variance"] = float(dev.max(initial=0.0))
    if wrong_cap.any():
        problems.append(f"variance above MAX_VARIANCE not clamped at {int(wrong_cap.sum())} pixels")
    # previous_spatial: which slots are written at all, and - where the winner stored on the validation branch - whose record it is.  A slot
    # a margin pixel aims at, or might have aimed at, is left out.
    doubtful = np.zeros(rw * rh, bool)
    aimed = r.slot[(r.margin | r.open) & (r.slot >= 0) & (r.slot < rw * rh)]
    doubtful[aimed] = True
    doubtful = doubtful.reshape(rh, rw) | r.margin | r.open
    written = (previous_spatial != PP.SENTINEL_U32).any(axis=-1)
    differs = (written != (r.winner >= 0)) & ~doubtful
    if differs.any():
        problems.append(f"previous_spatial written / left alone disagrees at {int(differs.sum())} slots, first {first(differs)}")
    # a background pixel's record has count 1 (set_reservoir), a refused history is stored as the empty record, count 0: who won a slot
    # that a background pixel owns, or one that only refused histories aim at, shows in the count
    wy, wx = np.divmod(np.maximum(r.winner, 0), rw)
    known = (r.winner >= 0) & ~doubtful & (r.background[wy, wx] | ~r.stored_second[wy, wx])
    want_count = np.where(r.background[wy, wx] & (planes.channel != 2), 0x3C00, 0)      # (indirect_lit_ambient stores the empty record for background too)
    differs = known & ((previous_spatial[..., 14] & 0xFFFF) != want_count)
    if differs.any():
        problems.append(f"previous_spatial holds the record of another kind of store at {int(differs.sum())} slots, first {first(differs)}")
    if r.second is not None:
        second = (r.winner >= 0) & r.stored_second[wy, wx] & ~r.background[wy, wx] & ~doubtful
        got = np.concatenate([halves(previous_spatial, 0), halves(previous_spatial, 1)], axis=-1)
        count = r.second["count"][wy, wx]
        whole = np.isfinite(count) & (count == np.floor(count)) & (count <= 2048.0)          # (a whole count is exact in f16)
        differs = second & ((got != r.second["radiance_bits"][wy, wx]).any(axis=-1) |
                            (previous_spatial[..., 4:8] != r.second["visible_position"][wy, wx].view(np.uint32)).any(axis=-1) |
                            (whole & ((previous_spatial[..., 14] & 0xFFFF) != PP.f16_bits(np.where(whole, count, 0.0)))))
        if differs.any():
            problems.append(f"previous_spatial holds another pixel's record at {int(differs.sum())} slots, first {first(differs)}")
    n_geometry = int(r.geometry.sum())
    share = float(((r.margin | r.open) & r.geometry).sum()) / n_geometry if n_geometry else 0.0
    return worst, share, r, problems


def channel_cases(name, channel, **settings):
    """every shape, ratio and frame numbers 2, 3 and 5 - 3 validates the sun, 5 the emitters at the default intervals; parities both"""
    for shape in SHAPES:
        for ratio in PP.SPATIAL_RATIOS:
            for frame_number in (2, 3, 5):
                yield PP.make_temporal_planes(name, 7, shape, ratio, channel, frame_number, scene="open", **settings)


# twice the worst deviation of the oracle from the restatement measured on `benign` per channel over every shape of SPATIAL_WIDTHS x
# SPATIAL_HEIGHTS, ratio and frame numbers 2, 3 and 5 (135 dispatches each), rounded up to the next whole ulp: `render`
# and the four statistics in f16 ulps, the variance in f32 ulps of the minuend w2_sum / count.  Measured:
#   sun       render 4.425   statistics 0.5001   variance 2.563
#   emissive  render 6.847   statistics 0.5001   variance 8.593
#   indirect  render 3.970   statistics 9.661    variance 2955.9   (w_new = luminance(shading) / pdf in f32, pdf = z / pi down to 2^-12, squared in w2_sum)
BOUNDS = {0: {"render": 9, "statistics": 2, "variance": 6}, 1: {"render": 14, "statistics": 2, "variance": 18}, 2: {"render": 8, "statistics": 20, "variance": 5912}}
EXCLUDED_CAP = 0.02
CHANNEL_IDS = pytest.mark.parametrize("channel", [0, 1, 2], ids=["sun", "emissive", "indirect"])


@pytest.fixture(scope="module")
def open_oracle(oracles):
    return oracles["open"]


@CHANNEL_IDS
def test_oracle_agrees_with_float64_on_benign(open_oracle, channel):
    """bounded on `benign` alone, per channel.  At most 2 % of a dispatch's geometry pixels may be left out as `margin` (rounded up to one whole
    pixel for small shapes) - the restatement alone decides that - and no pixel may be `open`; `benign` places no pixel, every one counts."""
    worst_all, failures = {}, []
    for planes in channel_cases("benign", channel):
        worst, share, r, problems = check(open_oracle, planes)
        n = int(r.geometry.sum())
        left_out = int(((r.margin | r.open) & r.geometry).sum())
        key = (planes.render_size, planes.ratio, int(planes.frame.number))
        if left_out > max(1, int(np.floor(EXCLUDED_CAP * n))) or r.open.any():
            failures.append((key, "left out", left_out, n))
        if problems:
            failures.append((key, problems))
        for k, v in worst.items():
            worst_all[k] = max(worst_all.get(k, 0.0), v)
            if v > BOUNDS[channel][k]:
                failures.append((key, k, v))
    print("worst deviation of the oracle from the float64 restatement on benign, channel", channel, worst_all)
    assert failures == []


#: what each planted mistake is run on: (set, frame number, settings) - planes on which the unplanted comparison is clean.  Frame 15
#: validates the sun and the emitters.
PLANTED = {"store_lt": ("edge", 2, {}), "depth_100": ("thresholds", 2, {}), "normal_0866": ("thresholds", 2, {}), "count_le_4": ("thresholds", 15, {}),
           "ratios_swapped": ("benign", 15, {}), "no_clamp": ("benign", 2, {"max_temporal_reuse_count": 4}), "visible_not_restored": ("scatter", 2, {}),
           "lowest_wins": ("scatter", 2, {})}
#: the planted mistakes that CANNOT show on a channel, with the reason: on the open scene the emissive pass's validation radiance is 0, its
#: luminance ratio 0 - below 0.8 and below 1.25 alike; indirect_lit_ambient has no validation frame, and every record it scatters, a
#: background pixel's included, is the empty record - whoever wins a slot, the bytes are the same
NOT_APPLICABLE = {0: (), 1: ("ratios_swapped",), 2: ("count_le_4", "ratios_swapped", "lowest_wins")}


@CHANNEL_IDS
@pytest.mark.parametrize("mistake", MISTAKES)
def test_the_comparison_notices_a_planted_mistake(open_oracle, mistake, channel):
    """`<` for `<=` in the store condition, 1.05 -> 1.0, 0.9 -> 0.866, `count < 4` -> `<= 4`, 1.25 / 0.8 swapped, the clamp omitted, the
    visible position not restored, lowest index wins: each must fail the comparison that passes without it, on the same planes, on every
    channel on which it can show (NOT_APPLICABLE: there the planted restatement must equal the clean one - the claim is checked too)"""
    name, frame_number, settings = PLANTED[mistake]
    bounded = name == "benign"
    fails = lambda worst, problems: bool(problems) or (bounded and any(v > BOUNDS[channel][k] for k, v in worst.items()))
    planes = PP.make_temporal_planes(name, 7, (70, 45), 1.5, channel, frame_number, scene="open", **settings)
    worst, _, _, problems = check(open_oracle, planes)
    assert not fails(worst, problems), (worst, problems)
    worst, _, _, problems = check(open_oracle, planes, mistake)
    assert fails(worst, problems) == (mistake not in NOT_APPLICABLE[channel]), (mistake, worst, problems)


# what the PASS decides on each set, from the restatement's replay of its decisions: a set that stops hitting its threshold fails here
DECIDED = {
    "benign": ["history_taken", "sample_merged"],
    "edge": ["history_taken", "refused_depth_alone", "refused_normal_alone", "refused_instance_alone", "outside", "store_discarded", "store_scattered", "store_to_own_slot"],
    "thresholds": ["history_taken", "refused_depth_alone", "refused_normal_alone", "refused_instance_alone", "background", "clamp_hit", "sample_merged"],
    "records": ["history_taken", "sample_merged"],
    "scatter": ["store_scattered", "store_to_own_slot", "history_taken", "refused_depth_alone", "background"],
    "background": ["background", "history_taken"],
    "random": ["background", "outside", "store_discarded", "store_scattered", "refused_depth_alone", "refused_instance_alone", "history_taken", "clamp_hit"],
}
#: ... and what only a pass with a validation frame, or with a lit sample, can decide
DECIDED_MORE = {
    0: {"benign": ["sample_picked", "validation_traced", "validation_replaced", "validation_kept", "store_to_own_slot"], "thresholds": ["validation_traced", "validation_replaced", "validation_kept"],
        "records": ["validation_replaced", "validation_kept", "sample_picked"], "scatter": ["validation_replaced"]},
    1: {"benign": ["validation_replaced", "store_to_own_slot"], "thresholds": ["validation_replaced"], "records": ["validation_replaced"], "scatter": ["validation_replaced"]},
    2: {"benign": ["sample_picked"], "records": ["sample_picked"]},
}


@CHANNEL_IDS
@pytest.mark.parametrize("name", PP.TEMPORAL_SETS)
def test_every_set_takes_the_branches_it_was_built_for(name, channel):
    """per-outcome pixel counts of each pass at 70 x 45, every ratio, frames 2, 3 and 5 together (3 validates the sun, 5 the emitters),
    clamp limit 4 for `thresholds` and `random` (their clamp pixels carry counts around the limit)"""
    extra = {"max_temporal_reuse_count": 4} if name in ("thresholds", "random") else {}
    for ratio in PP.SPATIAL_RATIOS:
        counts = {}
        for frame_number in (2, 3, 5):
            r = restate(PP.make_temporal_planes(name, 7, (70, 45), ratio, channel, frame_number, scene="open", **extra))
            for k, v in r.branches.items():
                counts[k] = counts.get(k, 0) + int(v.sum())
        want = DECIDED[name] + DECIDED_MORE[channel].get(name, [])
        assert [k for k in want if not counts.get(k)] == [], (ratio, counts)


def test_the_thresholds_set_lands_on_both_sides_of_each_decision():
    """at the placed pixels, by the restatement's decisions and with nothing within rounding: the normal bytes (55 + a, 0, 114) pass and
    fail against 0.9; counts 3 and 4 - one f16 step merge, 4 and 4 + one step do not (validation frame); the clamp limit minus one stays,
    the limit and the limit plus one are clamped; the luminance levels either side of 1.25 and of 0.8 keep and replace; random.x of the depth
    pixels comes within 0.01 of 0, of 1 and of one half (it is the noise tile's: exactly 0 and 65535 / 65535 are not on offer)"""
    for ratio in PP.SPATIAL_RATIOS:
        p2, p3 = (PP.make_temporal_planes("thresholds", 7, (70, 45), ratio, 0, n, scene="open", max_temporal_reuse_count=20) for n in (2, 3))
        r2, r3 = restate(p2), restate(p3)
        at = lambda plane, what, planes: np.array([plane[y, x] for x, y in planes.where[what]])
        assert not at(r2.reasons["normal"], "normal", p2).any() and not at(r3.reasons["luminance"], "luminance", p3).any()
        refused = at(r2.branches["refused_normal_alone"], "normal", p2)
        assert refused.any() and not refused.all()
        merged = at(r3.branches["sample_merged"], "count", p3)
        bits = np.array([p3.previous.count[y, x] for x, y in p3.where["count"]])
        four = int(PP.f16_bits(4.0))
        assert {int(b) for b in bits} == {int(PP.f16_bits(3.0)), four - 1, four, four + 1} and (merged == (bits < four)).all()
        clamped = at(r2.branches["clamp_hit"], "clamp", p2)
        counts = np.array([float(np.uint16(p2.previous.count[y, x]).view(np.float16)) for x, y in p2.where["clamp"]])
        assert set(counts) == {10.0, 19.0, 20.0, 21.0} and (clamped == (counts + 1.0 > 20.0)).all()
        levels = {int(p3.previous.radiance[y, x, 0]): bool(r3.branches["validation_replaced"][y, x]) for x, y in p3.where["luminance"]}
        for target in ("1.25", "0.8"):
            above, below = int(PP.luminance_level(p3, target, "above")), int(PP.luminance_level(p3, target, "below"))
            assert levels[above] != levels[below] and levels[above] == (target == "1.25")
        rx = np.array([float(PP.temporal_random_x(p2, x, y)) for x, y in p2.where["depth"]])
        assert rx.min() < 0.01 and rx.max() > 0.99 and np.abs(rx - 0.5).min() < 0.01
        # (their depths sit one f32 ulp either side of the threshold - within rounding for float64, so `margin` here: the f32 replay of
        # test_the_depth_threshold_pixels_sit_one_ulp_either_side holds their four outcomes)
        assert at(r2.reasons["depth"], "depth", p2).all()


@CHANNEL_IDS
def test_every_slot_the_restatement_forms_is_in_range_or_discarded(channel):
    """the index property from the restatement, per channel: over all sets, shapes and ratios a pixel that stores has a slot in [0, rw * rh),
    or the restatement counts its store as discarded and it wins no slot; `edge` discards at least one store in every shape"""
    for name in PP.TEMPORAL_SETS:
        for k, shape in enumerate(SHAPES):
            # (the sets that move nothing form the pixel's own slot at every ratio, and the emissive and indirect passes form the slots the
            # sun's does: they take the ratios in turn)
            every = name in ("edge", "scatter", "random") and channel == 0
            for ratio in (PP.SPATIAL_RATIOS if every else PP.SPATIAL_RATIOS[k % 3:k % 3 + 1]):
                p = PP.make_temporal_planes(name, 7, shape, ratio, channel, 2 + (k + int(2 * ratio)) % 2 + 3 * (channel == 1), scene="open")
                rw, rh = p.render_size
                r = restate(p)
                wants = r.branches["store_discarded"] | r.branches["store_scattered"] | r.branches["store_to_own_slot"]
                assert (r.slot[wants] >= 0).all() and ((r.slot[wants] < rw * rh) | r.branches["store_discarded"][wants]).all()
                assert not (r.branches["store_discarded"] & (r.slot < rw * rh)).any()
                assert (r.winner < rw * rh).all()
                lost = r.branches["store_discarded"]
                assert not np.isin(r.winner.ravel(), np.flatnonzero(lost.ravel())).any()       # (both stores of a pixel aim at one slot)
                if name == "edge":
                    assert lost.any(), (shape, ratio)
                    if rw > 1 and rh > 1:                              # ... and keeps a store that wraps into the next row
                        _, counts, unloaded = PP.temporal_store_targets(p)
                        assert (unloaded & r.branches["store_scattered"]).any(), (shape, ratio)
                elif name != "random":
                    assert not lost.any(), (name, shape, ratio)
