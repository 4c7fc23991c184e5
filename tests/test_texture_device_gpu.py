"""Texture edits from device memory (hk_update_textures_device, hk_read_texture) on the small textured yard.  The yardsticks: a TWIN
context that gets the same bytes - hk_encode_texels of the same values - through hk_update_texture / hk_upload_textures, the CPU oracle
given upload_textures, and hk_read_texture against a host model of every texture.  Every comparison is byte for byte."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import SceneData, texture_source
from bevy_hikari_amd.scenes import synthetic_camera
from test_device_refit import pose, refit_nodes
from test_texture_update_gpu import CHECKER, GLOW, NOISE, STRIPES, contexts, render_and_compare

pytestmark = pytest.mark.gpu
DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}


def torch_():
    import torch

    return torch


def to_device(array):
    """a torch tensor on cuda:0 with the values AND the strides of `array` (a numpy view: its base goes to the device whole)"""
    torch = torch_()
    root = array
    while isinstance(root.base, np.ndarray):
        root = root.base
    assert root.flags.c_contiguous and root.dtype == array.dtype
    whole = torch.from_numpy(root.reshape(-1)).to("cuda:0")
    elem = array.itemsize
    offset = array.ctypes.data - root.ctypes.data
    return whole.as_strided(array.shape, tuple(s // elem for s in array.strides), offset // elem)


def values(rng, dtype, shape):
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(-0.1, 1.1, shape).astype(dtype)


class Model:
    """the host's picture of every texture: what the twin and the oracle are given, what hk_read_texture must return"""

    def __init__(self, textures):
        self.textures = [dict(t, rgba=np.array(t["rgba"], dtype=np.uint8)) for t in textures]

    def apply(self, items):
        """items as Engine.update_textures takes them, with `array` (numpy) in place of `tensor`; returns the textures touched"""
        for it in items:
            t = self.textures[it["index"]]
            for key, mine in (("srgb", "srgb"), ("filter", "linear"), ("address_u", "address_u"), ("address_v", "address_v")):
                if key in it:
                    t[mine] = it[key]
        for it in items:
            t = self.textures[it["index"]]
            enc = hk.encode_texels(it["array"], it.get("layout", "hwc"), linear=it.get("linear", False), texture_srgb=t["srgb"])
            x0, y0 = it.get("origin", (0, 0))
            t["rgba"] = t["rgba"].copy()
            t["rgba"][y0:y0 + enc.shape[0], x0:x0 + enc.shape[1]] = enc
        return sorted({it["index"] for it in items})


def device_items(items):
    return [dict({k: v for k, v in it.items() if k != "array"}, tensor=to_device(it["array"])) for it in items]


def frame_edits(rng):
    """{frame: items}: the sRGB emissive texture from a float32 CHW tensor of linear light; the bilinear checker from a uint8 HWC tensor
    with a nearest / mirror sampler; a 5 x 3 rectangle at an odd origin of the noise texture from float16; three textures in one call"""
    return {
        2: [dict(index=GLOW, array=rng.uniform(0.05, 1.0, (3, 4, 16)).astype(np.float32), layout="chw", linear=True)],
        3: [dict(index=CHECKER, array=values(rng, np.uint8, (16, 32, 4)), filter=False, address_u=F.ADDRESS_MIRROR_REPEAT, address_v=F.ADDRESS_MIRROR_REPEAT)],
        4: [dict(index=NOISE, array=values(rng, np.float16, (3, 5, 4)), origin=(3, 7))],
        5: [dict(index=STRIPES, array=values(rng, np.uint8, (3, 8, 8)), layout="chw"),
            dict(index=GLOW, array=rng.uniform(0.0, 1.0, (2, 7, 3)).astype(np.float32), origin=(5, 1), linear=True),
            dict(index=CHECKER, array=values(rng, np.float16, (16, 32)), srgb=False)],
    }


@pytest.mark.parametrize("moving", [False, True])
def test_one_edit_per_frame_equals_the_twin_and_the_oracle(moving):
    """moving: a device refit of three instances between the frames, where hk_upload_textures is refused on the device context; the
    oracle and the twin get the host builder's records for the same poses (tests/test_texture_update_gpu.py)."""
    gpu, cpu, twin, scene, ref_scene, sun = contexts()
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    model = Model(scene.textures)
    edits = frame_edits(np.random.default_rng(23))
    rest = np.array([np.ctypeslib.as_array(i.model).copy() for i in ref_scene.instances], dtype=np.float32)
    current, movers = rest.copy(), [1, 4, len(rest) - 1]
    for n in range(1, 6):
        if n > 1:
            if moving:
                previous = current.copy()
                for k, i in enumerate(movers):
                    current[i] = pose(rest[i], n - 1, k)
                    for b in (scene.builder, ref_scene.builder):
                        b.set_instance_transform(i, current[i])
                assert gpu.engine.refit_instances(scene.builder) == len(movers)
                new = ref_scene.builder.finish()
                boxes = np.array([[list(i.min), list(i.max)] for i in new.instances], dtype=np.float32)
                eboxes = np.array([[[e.position[k] - e.radius for k in range(3)], [e.position[k] + e.radius for k in range(3)]] for e in new.emissives], dtype=np.float32)
                expected = SceneData(previous_transforms=previous, vertices=new.vertices, primitives=new.primitives, asset_nodes=new.asset_nodes, materials=new.materials,
                                     instances=new.instances, instance_nodes=refit_nodes(ref_scene.instance_nodes, boxes), emissives=new.emissives,
                                     emissive_nodes=refit_nodes(ref_scene.emissive_nodes, eboxes), alias_table=new.alias_table)
            gpu.update_textures(device_items(edits[n]))
            assert gpu.engine.last_texture_update()[:2] == (len(edits[n]), 1)      # one launch however many items (the issue allows two)
            touched = model.apply(edits[n])
            cpu.engine.upload_textures(model.textures)
            if moving:
                twin.engine.upload_textures(model.textures)
                for p in (cpu, twin):
                    p.update_instances(expected)
            else:
                for index in touched:
                    twin.engine.update_texture(index, model.textures[index])
        render_and_compare((gpu, cpu, twin), n, cam, lights, "moving: " if moving else "")
    for index, t in enumerate(model.textures):
        assert np.array_equal(gpu.read_texture(index), t["rgba"]), index
    assert gpu.engine.stats().scene_device_refits == (4 if moving else 0)


PLACEMENT = {   # per extra texture (width, height): the rectangles (x0, y0, w, h) - whole, 1 x 1, 1 x h, w x 1, odd origin with odd width
    4: ((7, 5), [(0, 0, 7, 5), (3, 2, 1, 1), (6, 0, 1, 5), (0, 4, 7, 1), (1, 1, 5, 3)]),
    5: ((13, 9), [(0, 0, 13, 9), (12, 8, 1, 1), (0, 0, 1, 9), (0, 8, 13, 1), (3, 1, 9, 7)]),
}


def test_placement_heads_tails_and_neighbours():
    """Six textures, the last starting at a texel offset that is no multiple of 4 (931).  Every format and layout writes whole textures
    and the smallest rectangles; after every call hk_read_texture of EVERY texture equals the model: the written ones changed exactly in
    the rectangle, the neighbours untouched to the byte.  The first call also lays out the pending hk_upload_textures."""
    gpu, _, twin, scene, _, sun = contexts()
    rng = np.random.default_rng(31)
    six = list(scene.textures) + [dict(rgba=values(rng, np.uint8, (h, w, 4)), srgb=k == 4, linear=True, address_u=F.ADDRESS_REPEAT, address_v=F.ADDRESS_REPEAT)
                                  for k, ((w, h), _) in PLACEMENT.items()]
    assert sum(t["rgba"].shape[0] * t["rgba"].shape[1] for t in six[:5]) % 4 != 0
    model = Model(six)
    for p in (gpu, twin):
        p.engine.upload_textures(six)
    e = gpu.engine

    def run(items, what):
        e.update_textures(device_items(items))
        model.apply(items)
        for index, t in enumerate(model.textures):
            assert np.array_equal(e.read_texture(index), t["rgba"]), f"{what}: texture {index}"

    step = 0
    for name, dtype in DTYPES.items():
        for layout in ("hwc", "chw"):
            for r in range(5):
                items = []
                for index, (_, rects) in PLACEMENT.items():
                    x0, y0, w, h = rects[r]
                    c = (1, 3, 4)[(step + index) % 3]
                    step += 1
                    items.append(dict(index=index, array=values(rng, dtype, (h, w, c) if layout == "hwc" else (c, h, w)), layout=layout, origin=(x0, y0),
                                      linear=dtype != np.uint8 and step % 2 == 0))
                run(items, f"{name} {layout} rectangle {r}")
    # a stride-0 source (one row for every row, one value for every channel) and a slice of a wider tensor
    row = values(rng, np.float32, (1, 13, 1))
    wide = values(rng, np.float16, (5, 20, 4))
    planes = values(rng, np.uint8, (4, 9, 40))
    run([dict(index=5, array=np.broadcast_to(row, (9, 13, 3))), dict(index=4, array=wide[:, 6:13, :])], "stride 0 and a column slice")
    run([dict(index=5, array=planes[:, :, 11:24], layout="chw"), dict(index=NOISE, array=np.broadcast_to(values(rng, np.float32, (1, 1, 1)), (4, 4, 4)), origin=(11, 5))],
        "a slice of planes and a constant")
    # ... and the scene still renders what the twin renders from the same bytes
    twin.engine.upload_textures(model.textures)
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    render_and_compare((gpu, twin), 1, cam, lights)


def test_the_producer_stream_is_ordered_before_and_after_the_call():
    torch = torch_()
    gpu, _, twin, scene, _, sun = contexts()
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    render_and_compare((gpu, twin), 1, cam, lights)
    model = Model(scene.textures)
    first = np.random.default_rng(41).uniform(0.0, 1.0, (16, 32, 4)).astype(np.float32)
    half = torch.from_numpy(first * np.float32(0.5)).to("cuda:0")    # (x 2 on the device is exact)
    busy = torch.randn((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream("cuda:0")
    with torch.cuda.stream(stream):
        for _ in range(8):                                            # the producing kernel is queued behind work that takes a while
            busy = torch.mm(busy, busy) * 1e-3
        texels = half * 2.0
        gpu.update_textures([dict(index=CHECKER, tensor=texels, linear=True)], producer_stream=stream)
        texels.fill_(0.123)                                           # overwritten in stream order right after the call
    model.apply([dict(index=CHECKER, array=first, linear=True)])
    assert np.array_equal(gpu.read_texture(CHECKER), model.textures[CHECKER]["rgba"])
    twin.engine.update_texture(CHECKER, model.textures[CHECKER])
    render_and_compare((gpu, twin), 2, cam, lights)
    torch.cuda.synchronize()


def test_refusals_write_nothing():
    """Every HK_E_INVALID of the list; the pointer cases rely on validation before any launch: nothing here may be made to fault."""
    torch = torch_()
    gpu, _, twin, scene, _, sun = contexts()
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    render_and_compare((gpu, twin), 1, cam, lights)
    e, api = gpu.engine, gpu.engine.api
    call = api.raw("update_textures_device")
    bytes_ = torch.zeros((16, 32, 4), dtype=torch.uint8, device="cuda:0")
    floats = torch.zeros((16, 32, 4), dtype=torch.float32, device="cuda:0")
    host = np.zeros((16, 32, 4), np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
    block, size = C.c_void_p(), 1 << 21
    assert hip.hipMalloc(C.byref(block), size) == 0

    def item(tensor=bytes_, index=CHECKER, **kw):
        s = texture_source(index, tensor)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    sampler = dict(flags=F.TEXTURE_SET_SAMPLER, is_srgb=1, filter_linear=1, address_u=0, address_v=0)
    cases = {
        "an index = the uploaded count": [item(index=len(scene.textures))],
        "an unknown format": [item(format=3)],
        "an unknown flag bit": [item(flags=4)],
        "two channels": [item(channels=2)],
        "an empty rectangle (width)": [item(width=0)],
        "an empty rectangle (height)": [item(height=0)],
        "a rectangle that leaves the texture in x": [item(x0=1)],
        "a rectangle that leaves the texture in y": [item(y0=15, height=2)],
        "an origin beyond 2^31": [item(x0=0xFFFFFFFF, width=2)],
        "a stride that is no multiple of the element size": [item(floats, stride_x=18)],
        "address_u out of range": [item(**dict(sampler, address_u=3))],
        "address_v out of range": [item(**dict(sampler, address_v=3))],
        "LINEAR_SOURCE on 8-bit texels": [item(flags=F.TEXTURE_LINEAR_SOURCE)],
        "two overlapping rectangles of one texture": [item(width=4, height=4), item(index=STRIPES, width=2, height=2), item(x0=3, y0=3, width=4, height=4)],
        "a pageable host pointer": [item(data=host.ctypes.data)],
        "a pointer 1 element before the end of its allocation, 2 x 2": [item(data=block.value + size - 1, width=2, height=2, channels=1, stride_x=1, stride_y=2, stride_c=0)],
        "a misaligned pointer": [item(floats, data=floats.data_ptr() + 2)],
        "NULL data": [item(data=None)],
    }
    n = 2
    for what, items in cases.items():
        table = (F.HkTextureSource * len(items))(*items)
        assert call(e.ctx, table, len(items), None) == F.HK_E_INVALID, what
        assert api.last_error(), what
        assert e.last_texture_update() == (0, 0, 0), what                 # nothing was ever enqueued
        render_and_compare((gpu, twin), n, cam, lights, f"after {what}: ")
        n += 1
    assert call(e.ctx, None, 1, None) == F.HK_E_INVALID
    assert call(e.ctx, None, 0, None) == F.HK_OK and e.last_texture_update() == (0, 0, 0)   # n == 0: nothing enqueued
    for index, t in enumerate(scene.textures):
        assert np.array_equal(e.read_texture(index), t["rgba"]), index
    bare = hk.Engine(device=0)                                            # no textures uploaded
    one = (F.HkTextureSource * 1)(item())
    assert call(bare.ctx, one, 1, None) == F.HK_E_NOT_READY
    assert api.raw("read_texture")(bare.ctx, 0, host.ctypes.data, host.size) == F.HK_E_NOT_READY
    torch.cuda.synchronize()
    assert hip.hipFree(block) == 0
    render_and_compare((gpu, twin), n, cam, lights, "after the refusals: ")


def test_the_host_calls_work_after_a_device_edit():
    """hk_update_texture of the same texture and hk_upload_textures both work after a device edit (no call is newly refused), and
    hk_read_texture checks its size."""
    gpu, _, twin, scene, _, sun = contexts()
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    rng = np.random.default_rng(53)
    model = Model(scene.textures)
    edit = [dict(index=CHECKER, array=values(rng, np.float32, (16, 32, 3)), linear=True), dict(index=NOISE, array=values(rng, np.uint8, (4, 16, 16)), layout="chw")]
    gpu.update_textures(device_items(edit))
    for index in model.apply(edit):
        twin.engine.update_texture(index, model.textures[index])
    render_and_compare((gpu, twin), 1, cam, lights)
    api, e = gpu.engine.api, gpu.engine
    out = np.zeros((16, 32, 4), np.uint8)
    read = api.raw("read_texture")
    assert read(e.ctx, CHECKER, out.ctypes.data, out.size - 4) == F.HK_E_INVALID and read(e.ctx, CHECKER, out.ctypes.data, out.size + 4) == F.HK_E_INVALID
    assert read(e.ctx, len(scene.textures), out.ctypes.data, out.size) == F.HK_E_INVALID and read(e.ctx, CHECKER, None, out.size) == F.HK_E_INVALID
    # hk_update_texture of the texture the device edited: its copy is refreshed, the other stale one stays the device's
    model.textures[CHECKER] = dict(model.textures[CHECKER], rgba=values(rng, np.uint8, (16, 32, 4)), linear=False)
    for p in (gpu, twin):
        p.engine.update_texture(CHECKER, model.textures[CHECKER])
    render_and_compare((gpu, twin), 2, cam, lights)
    assert np.array_equal(e.read_texture(NOISE), model.textures[NOISE]["rgba"]) and np.array_equal(e.read_texture(CHECKER), model.textures[CHECKER]["rgba"])
    # a device edit, then hk_upload_textures of everything: the stale copies are replaced
    again = [dict(index=GLOW, array=values(rng, np.float16, (4, 16, 4)), linear=True, address_u=F.ADDRESS_MIRROR_REPEAT)]
    gpu.update_textures(device_items(again))
    model.apply(again)
    twin.engine.update_texture(GLOW, model.textures[GLOW])
    render_and_compare((gpu, twin), 3, cam, lights)
    model.textures[STRIPES] = dict(model.textures[STRIPES], rgba=values(rng, np.uint8, (8, 8, 4)))
    for p in (gpu, twin):
        p.engine.upload_textures(model.textures)
    render_and_compare((gpu, twin), 4, cam, lights)
    for index, t in enumerate(model.textures):
        assert np.array_equal(e.read_texture(index), t["rgba"]), index
    # ... and a device edit while an hk_upload_textures is still pending: the call lays the scene out first
    gpu.engine.upload_textures(model.textures)
    last = [dict(index=STRIPES, array=values(rng, np.uint8, (8, 8)))]
    gpu.update_textures(device_items(last))
    model.apply(last)
    twin.engine.update_texture(STRIPES, model.textures[STRIPES])
    render_and_compare((gpu, twin), 5, cam, lights)
