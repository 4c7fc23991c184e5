"""k_smaa_tu4x, k_smaa_tu4x_extrapolate, k_taa_jasmine, k_fsr_easu and k_fsr_rcas on the adversarial planes of
tests/post_planes.py (`make_aa_planes`), bit for bit against the oracle: pass by pass, each pass alone on a written input, through
hk_frame_stage, in row ranges that cut through a workgroup, after the host rewrote the previous frame's G-buffer, and against what
the reference's own shaders wrote on the planes (the committed fixtures of tests/tools/wgsl_pin.py --aa-planes).

tests/test_aa_planes.py holds the oracle to a float64 restatement of all five shaders on these same planes;
through bit equality with the oracle its bounds hold for the kernels as well and are not measured again here."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
import post_planes as PP
from bevy_hikari_amd import _ffi as F
from cases import diff_buffers

pytestmark = pytest.mark.gpu

BUFS = {F.BUF_UPSCALE_OUTPUT: "upscale_output", F.BUF_TAA_OUTPUT: "taa_output", F.BUF_UPSCALE_SHARPENED: "upscale_sharpened"}
SHAPES = [(w, h) for w in PP.RENDER_WIDTHS for h in PP.RENDER_HEIGHTS]                 # render shapes of the 64 x 4 row kernels
FSR_WINDOWS = [(w, h) for w in PP.FSR_SIZES for h in (1, 15, 16, 17, 33)] + [(33, 130), (16, 130)]     # output shapes of the 16 x 16 tiles
SMAA, FSR = [s for s in PP.AA_SETTINGS if s.startswith("smaa")], [s for s in PP.AA_SETTINGS if s.startswith("fsr")]


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


def windows(setting):
    """the windows a setting is run at: every render shape, and for FSR1 every output shape of the tiled kernels as well"""
    w = [PP.aa_window_for(shape, setting) for shape in SHAPES]
    return w + (FSR_WINDOWS if setting in FSR else [])


def cases(setting):
    return [(window, parity) for window in windows(setting) for parity in (2, 3)]


@pytest.mark.parametrize("setting", list(PP.AA_SETTINGS))
@pytest.mark.parametrize("name", PP.AA_SETS)
def test_every_pass_equals_the_oracle(engines, name, setting):
    g, c = engines
    bad = {}
    for window, parity in cases(setting):
        planes = PP.make_aa_planes(name, 7, window, setting, parity)
        for e in engines:
            PP.install_aa(e, planes)
        for pass_id in planes.passes:
            for e in engines:
                e.pass_run(pass_id)
            d = diff_buffers(snapshot(g), snapshot(c))
            if d:
                bad[(window, parity, F.PASS_NAMES[pass_id])] = d
                break
    assert bad == {}


@pytest.mark.parametrize("setting", ["smaa2_taa", "smaa1_taa", "fsr10_taa", "fsr15_taa", "fsr20"])
@pytest.mark.parametrize("name", PP.AA_SETS)
def test_passes_alone_on_a_written_input_equal_the_oracle(engines, name, setting):
    """The extrapolate pass and TAA on a written `upscale_output` (SMAA Tu4x), RCAS on a written EASU output (FSR1): in the chain
    these read what the pass before them wrote, which is finite where that pass clamps.  Written, the input brings NaN, the
    infinities and the flat patches at 0 and 1 to every tap."""
    g, c = engines
    bad = {}
    alone = [F.PASS_SMAA_TU4X_EXTRAPOLATE, F.PASS_TAA_JASMINE] if setting in SMAA else [F.PASS_FSR_RCAS]
    for window, parity in cases(setting):
        planes = PP.make_aa_planes(name, 7, window, setting, parity)
        for pass_id in alone:
            for e in engines:
                PP.install_aa(e, planes)
                e.pass_run(pass_id)
            d = diff_buffers(snapshot(g), snapshot(c))
            if d:
                bad[(window, parity, F.PASS_NAMES[pass_id])] = d
    assert bad == {}


@pytest.mark.parametrize("setting", list(PP.AA_SETTINGS))
@pytest.mark.parametrize("name", PP.AA_SETS)
def test_the_stages_equal_the_oracle_and_the_passes(engines, name, setting):
    g, c = engines
    bad = {}
    for window in [PP.aa_window_for(shape, setting) for shape in ((130, 17), (65, 9), (63, 17), (64, 1), (1, 9))]:
        for parity in (2, 3):
            planes = PP.make_aa_planes(name, 7, window, setting, parity)
            for e in engines:
                PP.install_aa(e, planes)
                e.frame_stage(F.STAGE_ANTIALIAS, planes.settings.to_c())
                e.frame_stage(F.STAGE_UPSCALE, planes.settings.to_c())
            staged = snapshot(g)
            d = diff_buffers(staged, snapshot(c))
            PP.install_aa(g, planes)
            for pass_id in planes.passes:
                g.pass_run(pass_id)
            d.update({"passes:" + k: v for k, v in diff_buffers(staged, snapshot(g)).items()})
            if d:
                bad[(window, parity)] = d
    assert bad == {}


@pytest.mark.parametrize("setting", list(PP.AA_SETTINGS))
@pytest.mark.parametrize("name", ["hdr", "depth", "random"])
def test_row_ranges_that_cut_a_workgroup_write_the_same_bytes(engines, name, setting):
    """Cuts at 1, at 6 and at height - 1 land inside a workgroup (64 x 4 rows, 16 x 16 tiles), issued last piece first.  The SMAA pair:
    every piece of k_smaa_tu4x, then every piece of the extrapolate pass - that one reads rows by - 1 and by + 2, which the first
    pass of its neighbours wrote."""
    g, _ = engines
    bad = {}
    for shape in ((130, 17), (65, 9), (63, 17), (64, 17), (1, 9)):
        for parity in (2, 3):
            planes = PP.make_aa_planes(name, 7, PP.aa_window_for(shape, setting), setting, parity)
            PP.install_aa(g, planes)
            whole = []
            for pass_id in planes.passes:
                g.pass_run(pass_id)
                whole.append(snapshot(g))
            PP.install_aa(g, planes)
            for k, pass_id in enumerate(planes.passes):
                rows = {F.PASS_SMAA_TU4X: planes.render_size, F.PASS_SMAA_TU4X_EXTRAPOLATE: planes.render_size, F.PASS_TAA_JASMINE: planes.taa_size,
                        F.PASS_FSR_EASU: planes.window_size, F.PASS_FSR_RCAS: planes.window_size}[pass_id][1]
                cuts = sorted({0, min(1, rows), min(6, rows), max(rows - 1, 0), rows})
                for y0, y1 in reversed(list(zip(cuts[:-1], cuts[1:]))):
                    g.pass_run(pass_id, 0, y0, y1)
                d = diff_buffers(whole[k], snapshot(g))
                if d:
                    bad[(shape, parity, F.PASS_NAMES[pass_id])] = d
                    break
    assert bad == {}


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("setting", ["smaa2_taa", "fsr15_taa"])
def test_a_rewritten_previous_gbuffer_reaches_the_kernels(engines, setting, staged):
    """TAA and SMAA Tu4x gather the previous frame's depths from a plane of their own, which follows the frame parity.  The host
    writes both position planes twice with no rendered frame in between: the second run must see the second DEPTHS, not only the
    second positions (the twin of test_a_rewritten_gbuffer_reaches_the_derived_planes, for the previous frame's plane)."""
    g, c = engines
    window = PP.aa_window_for((65, 17), setting)
    first, second = PP.make_aa_planes("depth", 7, window, setting, 3), PP.make_aa_planes("depth", 7, window, setting, 3)
    # only the DEPTHS of the two position planes change (what the kernels take from .xyz they read from the written plane itself):
    # the block without geometry gets a previous depth (has_content: no clear colour any more), the left third loses its geometry in
    # both frames (the clear colour), the rest of the previous frame moves away (a depth ratio of 0.5)
    w = window[0]
    now, before = second.buffers[F.BUF_POSITION], second.buffers[F.BUF_PREVIOUS_POSITION]
    empty = (now[..., 3] == 0.0) & (before[..., 3] == 0.0)
    before[..., 3] *= np.float32(2.0)
    before[empty, 3] = 1.0
    now[:, :w // 3, 3] = 0.0
    before[:, :w // 3, 3] = 0.0
    results = []
    for planes in (first, second):
        for e in engines:
            PP.install_aa(e, planes)
            if staged:
                e.frame_stage(F.STAGE_ANTIALIAS, planes.settings.to_c())
                e.frame_stage(F.STAGE_UPSCALE, planes.settings.to_c())
            else:
                for pass_id in planes.passes:
                    e.pass_run(pass_id)
        results.append(snapshot(g))
        assert diff_buffers(results[-1], snapshot(c)) == {}
    assert "taa_output" in diff_buffers(results[0], results[1])


def _fixtures():
    from test_aa_planes import AA_PLANES_FIXTURES

    return AA_PLANES_FIXTURES


@pytest.mark.parametrize("case", _fixtures(), ids=lambda c: f"{c[0]}-{c[1]}-f{c[3]}")
def test_gpu_equals_what_the_reference_shaders_wrote_on_the_planes(engines, case):
    """The kernels against the outputs of the reference's own taa.wgsl, smaa.wgsl and FSR_Pass.glsl on the planes
    (tests/golden/wgsl_aa_planes_*.npz), dispatch by dispatch - no oracle in between."""
    from test_aa_planes import replay_aa_planes

    assert replay_aa_planes(engines[0], case) == []


def test_a_previous_gbuffer_written_through_its_device_pointer_reaches_the_kernels(engines):
    """hk_device_ptr(HK_BUF_PREVIOUS_POSITION): the host writes the plane through the pointer and asks for it again (hikari_hip.h) -
    the next anti-aliasing dispatch must gather the depths it wrote, as after hk_write_buffer."""
    import ctypes

    g, c = engines
    setting = "smaa2_taa"
    planes = PP.make_aa_planes("depth", 7, PP.aa_window_for((65, 17), setting), setting, 3)
    for e in engines:
        PP.install_aa(e, planes)
    before = planes.buffers[F.BUF_PREVIOUS_POSITION].copy()
    before[..., 3] *= np.float32(2.0)                     # every depth ratio becomes 0.5
    c.write(F.BUF_PREVIOUS_POSITION, before)
    g.wait()
    pointer, _ = g.device_ptr(F.BUF_PREVIOUS_POSITION)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
    assert hip.hipMemcpy(pointer, before.ctypes.data, before.nbytes, 1) == 0          # hipMemcpyHostToDevice, synchronous
    g.device_ptr(F.BUF_PREVIOUS_POSITION)                 # "asks again after writing"
    for pass_id in planes.passes:
        for e in engines:
            e.pass_run(pass_id)
    assert diff_buffers(snapshot(g), snapshot(c)) == {}
