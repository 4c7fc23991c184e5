"""hk_present / Engine.present on the GPU, byte for byte against tests/present_ref.py (in the float formats a NaN matches any NaN):
the adversarial planes at the three shapes that take the kernel's sampling paths, every format x HDR x clear / kept target, a
pitched target with guard bytes, a row range, the three final buffers of a rendered Cornell frame, the ordering against the frames
around it, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
import present_ref as R
from bevy_hikari_amd import _ffi as F

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CLEAR = (0.125, 0.25, 0.5, 0.75)
# name: (window size, upscale ratio, target size) -> the source (the tone-mapped image) is ceil(window / ratio), the albedo the window
SHAPES = {"equal": ((37, 19), 1.0, (37, 19)),            # odd sizes, no multiple of a 64-lane row: both planes read at the texel
          "upscaled": ((37, 19), 1.55, (37, 19)),        # source 24 x 13 through the bilinear path, clamped edges, NaN footprints
          "albedo-differs": ((48, 26), 2.0, (24, 13))}   # source 24 x 13 at the texel, albedo 48 x 26 through the bilinear path
SOURCE_SIZE = {"equal": (37, 19), "upscaled": (24, 13), "albedo-differs": (24, 13)}


@pytest.fixture(scope="module")
def plugin():
    p = hk.HikariPlugin(device=0)
    p.set_scene(hk.load_cornell())
    return p


def install(engine, name):
    """hk_resize, hk_frame_begin, then the adversarial planes through hk_write_buffer -> (settings, source, albedo, W, H)"""
    window, ratio, (W, H) = SHAPES[name]
    settings = hk.HikariSettings(upscale=hk.Upscale.SmaaTu4x(ratio))
    engine.resize(*window, ratio)
    camera = hk.cornell_camera(*window)
    engine.frame_begin(hk.frame_uniform(settings, 2), camera.view_uniform(), camera.previous_view_uniform(None), hk.lights_uniform())
    assert engine.buffer_info(F.BUF_TONE_MAPPED)[:2] == SOURCE_SIZE[name] and engine.buffer_info(F.BUF_ALBEDO)[:2] == window
    src, albedo = R.make_planes(SOURCE_SIZE[name], window)
    engine.write(F.BUF_TONE_MAPPED, src)
    engine.write(F.BUF_ALBEDO, albedo)
    return settings, src, albedo, W, H


def tensor_of(array):
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_format_equals_the_reference(plugin, name):
    e = plugin.engine
    settings, src, albedo, W, H = install(e, name)
    bad = []
    for fmt in R.FORMATS:
        before = R.random_target(fmt, W, H)
        for hdr in (False, True):
            for clear in (CLEAR, None):
                out = tensor_of(before)
                got = e.present(settings, antialias=False, format=fmt, hdr=hdr, clear=clear, out=out)
                assert got is out
                want = R.present(src, albedo, W, H, fmt, hdr=hdr, clear=clear, target=before)
                if not R.same(out.cpu().numpy(), want):
                    bad.append((fmt, hdr, clear is not None))
    assert bad == []


def test_an_allocated_target_has_the_final_images_size(plugin):
    e = plugin.engine
    settings, src, albedo, _, _ = install(e, "upscaled")
    out = e.present(settings, antialias=False, format="rgba32f", clear=CLEAR)
    assert tuple(out.shape) == (13, 24, 4) and out.dtype == torch.float32 and out.is_cuda
    assert R.same(out.cpu().numpy(), R.present(src, albedo, 24, 13, "rgba32f", clear=CLEAR))


@pytest.mark.parametrize("fmt", ["bgra8-srgb", "rgba16f"])
def test_a_pitched_target_keeps_its_guard_bytes(plugin, fmt):
    e = plugin.engine
    settings, src, albedo, W, H = install(e, "upscaled")
    pixel = 4 if fmt == "bgra8-srgb" else 8
    row, pitch = W * pixel, W * pixel + 5 * pixel
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, size=H * pitch + 64, dtype=np.uint8)
    rows = raw[: H * pitch].reshape(H, pitch)
    before = rows[:, :row].copy().view(R.DTYPES[fmt]).reshape(H, W, 4)
    if fmt == "rgba16f":
        before = np.nan_to_num(before.astype(np.float32), nan=0.5).astype(np.float16)   # (random bits: keep the kept target's NaNs out of the guards' way)
        rows[:, :row] = before.view(np.uint8).reshape(H, row)
    dev = tensor_of(raw)
    e.present_into(settings.to_c(), 0, dev.data_ptr(), W, H, pitch, R.FORMATS[fmt], 0, None)
    e.wait()
    got = dev.cpu().numpy()
    got_rows = got[: H * pitch].reshape(H, pitch)
    assert (got_rows[:, row:] == rows[:, row:]).all() and (got[H * pitch:] == raw[H * pitch:]).all()
    want = R.present(src, albedo, W, H, fmt, target=before)
    assert R.same(np.ascontiguousarray(got_rows[:, :row]).view(R.DTYPES[fmt]).reshape(H, W, 4), want)


def test_a_row_range_leaves_the_other_rows_alone(plugin):
    e = plugin.engine
    settings, src, albedo, W, H = install(e, "equal")
    before = R.random_target("rgba8-srgb", W, H)
    out = e.present(settings, antialias=False, format="rgba8-srgb", hdr=True, clear=None, out=tensor_of(before), rows=(5, 11)).cpu().numpy()
    want = before.copy()
    want[5:11] = R.present(src, albedo, W, H, "rgba8-srgb", hdr=True, target=before)[5:11]
    assert (out == want).all()


@pytest.mark.parametrize("upscale,taa", [(hk.Upscale.Fsr1(2.0, 0.25), hk.Taa.Jasmine), (hk.Upscale.SmaaTu4x(2.0), hk.Taa.NONE),
                                         (hk.Upscale.SmaaTu4x(2.0), hk.Taa.Jasmine)], ids=["fsr1", "smaa", "smaa-jasmine"])
def test_a_rendered_frame_presents_its_final_buffer(upscale, taa):
    settings = hk.HikariSettings(upscale=upscale, taa=taa)
    p = hk.HikariPlugin(device=0)
    p.set_scene(hk.load_cornell())
    camera = hk.cornell_camera(64, 64)
    for _ in range(4):
        p.render(camera, settings, antialias=True)
    out = p.present(settings, antialias=True, format="rgba32f", clear=settings.clear_color)
    final = F.api().final_buffer(settings.to_c(), F.FRAME_ANTIALIAS)
    src, albedo = p.engine.read(final), p.engine.read(F.BUF_ALBEDO)
    assert final == {"fsr1": F.BUF_UPSCALE_SHARPENED, "smaa": F.BUF_UPSCALE_OUTPUT, "smaa-jasmine": F.BUF_TAA_OUTPUT}[
        "fsr1" if upscale.kind == F.UPSCALE_FSR1 else ("smaa" if taa == hk.Taa.NONE else "smaa-jasmine")]
    H, W = src.shape[:2]
    assert tuple(out.shape) == (H, W, 4) and np.isfinite(src.view(np.float16).astype(np.float32)).all() and src.any()
    assert R.same(out.cpu().numpy(), R.present(src, albedo, W, H, "rgba32f", clear=settings.clear_color))


@pytest.mark.parametrize("antialias", [False, True])
def test_presents_between_frames_need_no_host_wait(antialias):
    """render, present, render, present, render, present with nothing in between on a context with frame pipelining on (the default):
    no frame may overwrite what an earlier present still reads, and each present must see its own frame finished.  The THIRD frame is
    the first that writes the planes of the first frame's parity again (tone-mapped image, albedo): it is ordered behind the first
    present only through the event hk_present records behind itself on the post stream.  Run once each way."""
    settings = hk.HikariSettings(indirect_bounces=2)
    camera = hk.cornell_camera(96, 64)

    def sequence(wait):
        p = hk.HikariPlugin(device=0)
        p.set_scene(hk.load_cornell())
        p.render(camera, settings, antialias=antialias)      # (a frame of history, so that frame pipelining has a previous frame to run beside)
        p.engine.wait()
        w, h, _ = p.engine.buffer_info(F.api().final_buffer(settings.to_c(), F.FRAME_ANTIALIAS if antialias else 0))
        outs = [torch.zeros((h, w, 4), dtype=torch.float16, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        for out in outs:
            p.render(camera, settings, antialias=antialias)
            if wait:
                p.engine.wait()
            p.present(settings, antialias=antialias, format="rgba16f", clear=settings.clear_color, out=out, wait=wait)
        p.engine.wait()
        return [o.cpu().numpy() for o in outs]

    free, waited = sequence(False), sequence(True)
    assert not R.same(waited[0], waited[1]) and not R.same(waited[0], waited[2]) and np.isfinite(waited[2].astype(np.float32)).all()
    assert [R.same(f, w) for f, w in zip(free, waited)] == [True, True, True]


def test_refusals_leave_the_target_unchanged(plugin):
    e = plugin.engine
    settings, _, _, W, H = install(e, "equal")
    sc = settings.to_c()
    before = R.random_target("rgba8-srgb", W, H)
    dev = tensor_of(np.concatenate([before.reshape(-1), np.zeros(16, np.uint8)]))
    ptr = dev.data_ptr()

    def refused(code, engine=e, ptr=ptr, fmt=F.FORMAT_RGBA8_UNORM_SRGB, rows=None, pitch=W * 4, flags=F.PRESENT_CLEAR):
        with pytest.raises(hk.HikariError) as err:
            engine.present_into(sc, 0, ptr, W, H, pitch, fmt, flags, CLEAR, rows)
        assert err.value.code == code and str(err.value).split(": ", 1)[1].strip(), err.value

    refused(F.HK_E_INVALID, ptr=0)                               # NULL
    refused(F.HK_E_INVALID, ptr=ptr + 2)                         # misaligned for a 4-byte pixel
    refused(F.HK_E_INVALID, ptr=ptr + 4, fmt=F.FORMAT_RGBA16F, pitch=W * 8)   # ... and for an 8-byte one
    refused(F.HK_E_INVALID, fmt=4)                               # unknown format
    refused(F.HK_E_INVALID, rows=(0, H + 1))                     # row_end > height
    refused(F.HK_E_INVALID, pitch=W * 4 - 4)                     # a pitch shorter than a row
    refused(F.HK_E_INVALID, flags=4)                             # unknown flag
    fresh = hk.Engine(device=0)                                  # no frame yet
    fresh.upload_noise()
    refused(F.HK_E_NOT_READY, engine=fresh)
    fresh.resize(W, H, 1.0)
    refused(F.HK_E_NOT_READY, engine=fresh)
    e.set_band(0, 2)                                             # one band of two
    try:
        refused(F.HK_E_UNSUPPORTED)
    finally:
        e.set_band(0, 1)
    e.wait()
    assert (dev.cpu().numpy()[:-16].reshape(H, W, 4) == before).all()
    e.present_into(sc, 0, ptr, W, H, W * 4, F.FORMAT_RGBA8_UNORM_SRGB, F.PRESENT_CLEAR, CLEAR)   # (and the same call, accepted, does write)
    e.wait()
    assert not (dev.cpu().numpy()[:-16].reshape(H, W, 4) == before).all()


def test_the_cpp_example_presents_what_the_reference_computes(tmp_path):
    """examples/cornell --present: the C++ OverlayNode into a bgra8-sRGB target the example owns through HIP, against the reference
    applied to the planes of the same frames rendered through the Python host."""
    import os
    import subprocess

    from conftest import ROOT

    out = tmp_path / "present.bgra"
    r = subprocess.run([os.path.join(ROOT, "examples", "cornell"), "--size", "96", "64", "--frames", "3", "--bounces", "1", "--ratio", "2.0", "--antialias",
                        "--present", str(out)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, dtype=np.uint8).reshape(64, 96, 4)
    p = hk.HikariPlugin(device=0)
    p.set_scene(hk.load_cornell())
    s = hk.HikariSettings(indirect_bounces=1)
    for n in range(1, 4):
        p.render(hk.cornell_camera(96, 64), s, frame_number=n, antialias=True)
    src, albedo = p.engine.read(F.BUF_TAA_OUTPUT), p.engine.read(F.BUF_ALBEDO)
    assert (got == R.present(src, albedo, 96, 64, "bgra8-srgb", clear=s.clear_color)).all()
