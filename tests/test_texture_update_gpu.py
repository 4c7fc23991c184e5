"""One texture replaced in place on the device (hk_update_texture): every frame must equal, bit for bit, the CPU oracle given the full
new array with upload_textures AND a twin context that takes hk_upload_textures, the path that re-sends every image behind a host
wait.  Also between device refits (where hk_upload_textures is refused on the device context) and after every refusal."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import SceneData, image_desc
from bevy_hikari_amd.scenes import synthetic_camera, synthetic_scene
from cases import diff_buffers, snapshot
from test_device_refit import SMALL, oracle, pose, refit_nodes

pytestmark = pytest.mark.gpu
SETTINGS = dict(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)
CHECKER, STRIPES, NOISE, GLOW = 0, 1, 2, 3   # scenes._test_textures


def edits_of(textures, rng):
    """{frame: (index, new image)}: the emissive texture; the bilinear-repeat checker with other texels and a nearest / mirror sampler;
    the sRGB flag of the checker flipped (same texels: only the descriptor changes)."""
    glow = dict(textures[GLOW], rgba=rng.integers(30, 256, textures[GLOW]["rgba"].shape, dtype=np.uint8))
    glow["rgba"][..., 3] = 255
    checker = dict(textures[CHECKER], rgba=np.ascontiguousarray(textures[CHECKER]["rgba"][::-1, ::-1] // 2 + 60), linear=False,
                   address_u=F.ADDRESS_MIRROR_REPEAT, address_v=F.ADDRESS_MIRROR_REPEAT)
    linear_checker = dict(checker, srgb=False)
    return {2: (GLOW, glow), 3: (CHECKER, checker), 4: (CHECKER, linear_checker)}


def contexts():
    scene, sun = synthetic_scene(textured=True, **SMALL)
    ref_scene, _ = synthetic_scene(textured=True, **SMALL)
    twin_scene, _ = synthetic_scene(textured=True, **SMALL)
    gpu, twin = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER), hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    cpu = oracle()
    for p, sc in ((gpu, scene), (cpu, ref_scene), (twin, twin_scene)):
        p.set_scene(sc)
    return gpu, cpu, twin, scene, ref_scene, sun


def render_and_compare(plugins, n, cam, lights, what=""):
    s = hk.HikariSettings(**SETTINGS)
    for p in plugins:
        p.render(cam, s, lights=lights, frame_number=n)
    first = snapshot(plugins[0])
    for k, p in enumerate(plugins[1:]):
        bad = diff_buffers(first, snapshot(p))
        assert bad == {}, f"{what}frame {n}, against context {k + 1}: {bad}"


@pytest.mark.parametrize("moving", [False, True])
def test_one_texture_per_frame_equals_the_full_upload(moving):
    """moving: a device refit of three instances between the frames; the oracle and the twin get the host builder's records for the
    same poses on the old tree shapes (test_device_refit.py) through hk_upload_instances - the host's path."""
    gpu, cpu, twin, scene, ref_scene, sun = contexts()
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    textures = list(scene.textures)
    edits = edits_of(textures, np.random.default_rng(11))
    rest = np.array([np.ctypeslib.as_array(i.model).copy() for i in ref_scene.instances], dtype=np.float32)
    current, movers = rest.copy(), [1, 4, len(rest) - 1]   # a box, the sphere, the emitter
    for n in range(1, 5):
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
            index, image = edits[n]
            gpu.engine.update_texture(index, image)
            textures[index] = image
            for p in (cpu, twin):
                p.engine.upload_textures(textures)
                if moving:
                    p.update_instances(expected)
        render_and_compare((gpu, cpu, twin), n, cam, lights, "moving: " if moving else "")
    st = gpu.engine.stats()
    assert st.scene_device_refits == (3 if moving else 0)


def test_refusals_leave_the_next_frame_alone():
    gpu, cpu, twin, scene, _, sun = contexts()
    cam, lights = synthetic_camera(88, 60), hk.lights_uniform(directional=sun)
    render_and_compare((gpu, twin), 1, cam, lights)
    e, api = gpu.engine, gpu.engine.api
    good = scene.textures[CHECKER]
    h, w = good["rgba"].shape[:2]
    bad_mode = image_desc(good)
    bad_mode.address_v = 3
    no_pixels = image_desc(good)
    no_pixels.rgba8 = None
    cases = [(CHECKER, image_desc(dict(good, rgba=np.zeros((h, w + 1, 4), np.uint8)))),   # another width
             (CHECKER, image_desc(dict(good, rgba=np.zeros((h * 2, w, 4), np.uint8)))),   # another height
             (len(scene.textures), image_desc(good)),                                     # index = the uploaded count
             (0xFFFFFFFF, image_desc(good)),
             (CHECKER, bad_mode), (CHECKER, no_pixels), (CHECKER, None)]
    for n, (index, desc) in enumerate(cases):
        with pytest.raises(hk.HikariError) as err:
            api.call("update_texture", e.ctx, index, None if desc is None else C.byref(desc))
        assert err.value.code == F.HK_E_INVALID, (n, err.value.code)
        render_and_compare((gpu, twin), 2 + n, cam, lights, f"after refusal {n}: ")
    with pytest.raises(hk.HikariError) as err:
        api.call("update_texture", None, CHECKER, C.byref(image_desc(good)))
    assert err.value.code == F.HK_E_INVALID
    bare = hk.Engine(device=0)   # no textures uploaded
    with pytest.raises(hk.HikariError) as err:
        api.call("update_texture", bare.ctx, 0, C.byref(image_desc(good)))
    assert err.value.code == F.HK_E_NOT_READY
