"""k_demodulation, k_denoise<LEVEL, NCH, FFMASK> and k_tone_mapping on the adversarial planes of tests/post_planes.py, bit for bit
against the oracle: per pass (NCH = 1), fused (frame_stage: NCH = 2 / 3, the tone mapping fused into level 3), in row ranges that
cut through a workgroup, after the host rewrote the G-buffer (k_derive_planes), and against what the reference's own shaders
wrote on the planes (the committed fixtures of tests/tools/wgsl_pin.py --planes).

tests/test_post_chain_planes.py holds the oracle to a float64 restatement of the shaders within a measured bound of f16 ulps on
these same planes; through bit equality with the oracle that bound holds for the kernels as well and is not measured again here."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F
from cases import diff_buffers

pytestmark = pytest.mark.gpu

BUFS = {F.BUF_DENOISE_INTERNAL0 + i: f"internal{i}" for i in range(4)}
BUFS[F.BUF_DENOISE_INTERNAL_VARIANCE] = "internal_variance"
BUFS.update({F.BUF_DENOISE_RENDER0 + i: f"denoise_render{i}" for i in range(3)})
BUFS[F.BUF_TONE_MAPPED] = "tone_mapped"
SHAPES = [(w, h) for w in PP.RENDER_WIDTHS for h in PP.RENDER_HEIGHTS]
RATIO_PARITY = [(1.0, 2), (1.0, 3), (1.5, 2), (1.5, 3)]


@pytest.fixture(scope="module")
def engines():
    from oracle_lib import oracle_plugin

    scene = hk.load_cornell()
    gpu, cpu = hk.HikariPlugin(device=0), oracle_plugin()
    for p in (gpu, cpu):
        p.set_scene(scene)
    return gpu.engine, cpu.engine


def snapshot(e):
    return {name: e.read(buf) for buf, name in BUFS.items()}


def clear_outputs(e):
    for buf in BUFS:
        e.write(buf, np.zeros_like(e.read(buf)))


def chain(channels):
    """the dispatches of PostProcessNode::run, then tone mapping straight from the render planes"""
    steps = [(p, ch) for ch in range(channels) for p in (F.PASS_DEMODULATION, F.PASS_DENOISE_L0, F.PASS_DENOISE_L1, F.PASS_DENOISE_L2, F.PASS_DENOISE_L3)]
    return steps + [(F.PASS_TONE_MAPPING, 1), (F.PASS_TONE_MAPPING, 0)]


def planes_for(name, shape, ratio, parity, channels=3, seed=7):
    return PP.make_planes(name, seed, PP.window_for(shape, ratio), ratio, channels, parity)


@pytest.mark.parametrize("ratio,parity", RATIO_PARITY)
@pytest.mark.parametrize("name", PP.SETS)
def test_every_pass_equals_the_oracle(engines, name, ratio, parity):
    g, c = engines
    bad = {}
    for shape in SHAPES:
        planes = planes_for(name, shape, ratio, parity)
        for e in engines:
            PP.install(e, planes)
        for pass_id, arg in chain(3):
            for e in engines:
                e.pass_run(pass_id, arg)
            d = diff_buffers(snapshot(g), snapshot(c))
            if d:
                bad[(shape, F.PASS_NAMES[pass_id], arg)] = d
                break
    assert bad == {}


@pytest.mark.parametrize("ratio,parity", RATIO_PARITY)
@pytest.mark.parametrize("name", ["nonfinite", "thresholds", "black"])
def test_levels_on_written_inputs_equal_the_oracle(engines, name, ratio, parity):
    """Each level run directly on the demodulated planes - a level fed by the one before it sees finite values where that one skipped.
    `nonfinite`: a rejected centre with all eight taps rejected, and a good centre with ff_count = 0, at every level's step;
    `thresholds`: the `sum_w < 0.0001` fallback at every level; `black`: the lit texel is a tap at THAT level's step for exactly one
    lane of the wave next to it.  Also on an `internal_variance` plane holding NaN, a negative value and +Inf: a NaN
    `lum_denominator` must take the whole wave the long way.  (tests/test_post_chain_planes.py asserts per level that these
    branches run on the same planes.)"""
    g, c = engines
    bad = {}
    for shape in [(130, 17), (65, 9), (64, 17), (63, 17), (130, 1), (1, 17)]:
        planes = planes_for(name, shape, ratio, parity)
        for e in engines:
            PP.install(e, planes)
        for ch in range(3):
            for e in engines:
                e.pass_run(F.PASS_DEMODULATION, ch)
            demodulated = c.read(F.BUF_DENOISE_INTERNAL0)
            for variance in (None, planes.internal_variance):
                for level in range(4):
                    for e in engines:
                        e.write(F.BUF_DENOISE_INTERNAL0 + level, demodulated)
                        if variance is not None:
                            e.write(F.BUF_DENOISE_INTERNAL_VARIANCE, variance)
                        e.pass_run(F.PASS_DENOISE_L0 + level, ch)
                    d = diff_buffers(snapshot(g), snapshot(c))
                    if d:
                        bad[(shape, ch, level, variance is not None)] = d
    assert bad == {}


@pytest.mark.parametrize("channels", [2, 3])
@pytest.mark.parametrize("name", PP.SETS)
def test_fused_post_process_equals_the_oracle_and_the_passes(engines, name, channels):
    g, c = engines
    bad = {}
    for shape in SHAPES:
        for ratio, parity in RATIO_PARITY:
            planes = planes_for(name, shape, ratio, parity, channels)
            for e in engines:
                PP.install(e, planes)
                e.frame_stage(F.STAGE_POST_PROCESS, planes.settings.to_c())
            fused = snapshot(g)
            d = diff_buffers(fused, snapshot(c))
            PP.install(g, planes)
            for pass_id, arg in chain(channels)[:-1]:
                g.pass_run(pass_id, arg)
            d.update({"passes:" + k: v for k, v in diff_buffers(fused, snapshot(g)).items()})
            if d:
                bad[(shape, ratio, parity)] = d
    assert bad == {}


@pytest.mark.parametrize("name", PP.SETS)
def test_row_ranges_that_cut_a_workgroup_write_the_same_bytes(engines, name):
    """A workgroup covers 64 x 4 pixels: cuts at 1, at 6 and at height - 1 land inside one."""
    g, _ = engines
    bad = {}
    for shape, ratio, parity in [(s, r, p) for s in ((130, 17), (65, 9), (63, 17), (64, 17), (1, 9)) for r, p in RATIO_PARITY]:
        planes = planes_for(name, shape, ratio, parity)
        cuts = sorted({0, 1, 6, shape[1] - 1, shape[1]})
        PP.install(g, planes)
        clear_outputs(g)
        whole = []
        for pass_id, arg in chain(3):
            g.pass_run(pass_id, arg)
            whole.append(snapshot(g))
        PP.install(g, planes)
        clear_outputs(g)
        for k, (pass_id, arg) in enumerate(chain(3)):
            for y0, y1 in reversed(list(zip(cuts[:-1], cuts[1:]))):
                g.pass_run(pass_id, arg, y0, y1)
            d = diff_buffers(whole[k], snapshot(g))
            if d:
                bad[(shape, ratio, parity, F.PASS_NAMES[pass_id], arg)] = d
                break
    assert bad == {}


@pytest.mark.parametrize("fused", [False, True])
def test_a_rewritten_gbuffer_reaches_the_derived_planes(engines, fused):
    """k_derive_planes packs the normalised normal, the instance id and the depth once per frame.  The host writes the G-buffer twice
    with no rendered frame in between (hk_frame_begin alone leaves the derived planes as they are): the second run must see the
    second normals, depths and instance ids (derived_dirty)."""
    g, c = engines
    shape, ratio, parity = (65, 17), 1.5, 3
    first, second = planes_for("thresholds", shape, ratio, parity, seed=7), planes_for("thresholds", shape, ratio, parity, seed=8)
    for buf in (F.BUF_RENDER0, F.BUF_RENDER0 + 1, F.BUF_RENDER0 + 2, F.BUF_VARIANCE0, F.BUF_VARIANCE0 + 1, F.BUF_VARIANCE0 + 2, F.BUF_ALBEDO):
        second.buffers[buf] = first.buffers[buf]          # only the G-buffer changes
    results = []
    for planes in (first, second):
        for e in engines:
            PP.install(e, planes)
            if fused:
                e.frame_stage(F.STAGE_POST_PROCESS, planes.settings.to_c())
            else:
                for pass_id, arg in chain(3)[:-1]:
                    e.pass_run(pass_id, arg)
        results.append(snapshot(g))
        assert diff_buffers(results[-1], snapshot(c)) == {}
    assert set(diff_buffers(results[0], results[1])) >= {"denoise_render0", "denoise_render1", "denoise_render2", "tone_mapped"}


def _fixtures():
    from test_post_chain_planes import PLANES_FIXTURES

    return PLANES_FIXTURES


@pytest.mark.parametrize("case", _fixtures(), ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}-f{c[3]}")
def test_gpu_equals_what_the_reference_shaders_wrote_on_the_planes(engines, case):
    """The kernels against the outputs of the reference's own WGSL on the planes (tests/golden/wgsl_post_planes_*.npz), dispatch by
    dispatch - no oracle in between."""
    from test_post_chain_planes import replay_planes

    assert replay_planes(engines[0], case) == []
