"""Ray queries (hikari_hip.h hk_cast_rays / hk_cast_rays_device), the part that needs no GPU: the header, the library and the
binding agree; the argument refusals; Camera.ray_through against the oracle's prepass; and the inputs of the GPU tests
(tests/ray_ref.py) are sane - the reference's own walk and the float64 brute-force caster agree wherever float64 can decide."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bevy_hikari_amd as hk
import ray_ref as R
from bevy_hikari_amd import _ffi as F
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402  (its header parser: structs field for field, the C layout rules)


def test_header_library_and_binding_agree():
    api = G.parse_header()
    functions = {name: params for name, _ret, params in api["functions"]}
    assert [p[0] for p in functions["hk_cast_rays"]] == ["ctx", "rays", "n", "flags", "hits"]
    assert [p[0] for p in functions["hk_cast_rays_device"]] == ["ctx", "d_rays", "n", "flags", "d_hits"]
    for name in ("hk_cast_rays", "hk_cast_rays_device"):
        assert name in F.DECLARED_SYMBOLS and hasattr(F.api().dll, name)
        assert len(F._PRODUCT_ONLY[name[3:]]) == 5
    structs, lay = dict(api["structs"]), G.layout(api)
    for name, mirror, size in (("HkRay", F.HkRay, 32), ("HkRayHit", F.HkRayHit, 48)):
        assert lay[name][0] == C.sizeof(mirror) == size
        assert [f for f, _c, _d in structs[name]] == [f[0] for f in mirror._fields_]
    assert [(f, getattr(F.HkRay, f).offset) for f, _ in F.HkRay._fields_] == [("origin", 0), ("max_distance", 12), ("direction", 16), ("exclude_instance", 28)]
    assert [(f, getattr(F.HkRayHit, f).offset) for f, _ in F.HkRayHit._fields_] == [
        ("distance", 0), ("instance", 4), ("primitive", 8), ("material", 12), ("barycentric", 16), ("uv", 24), ("normal", 32), ("status", 44)]
    assert hk.RAY_DTYPE.itemsize == 32 and hk.HIT_DTYPE.itemsize == 48
    assert [hk.RAY_DTYPE.fields[f][1] for f, _ in F.HkRay._fields_] == [0, 12, 16, 28]
    assert [hk.HIT_DTYPE.fields[f][1] for f, _ in F.HkRayHit._fields_] == [0, 4, 8, 12, 16, 24, 32, 44]
    consts = G.const_values(api)
    assert (consts["HK_RAYS_CLOSEST"], consts["HK_RAYS_ANY"], consts["HK_RAYS_ATTRIBUTES"], consts["HK_RAYS_STACKLESS"]) == (F.RAYS_CLOSEST, F.RAYS_ANY, F.RAYS_ATTRIBUTES, F.RAYS_STACKLESS) == (0, 1, 2, 4)
    assert (consts["HK_RAY_MISS"], consts["HK_RAY_HIT"], consts["HK_RAY_INVALID"]) == (F.RAY_MISS, F.RAY_HIT, F.RAY_INVALID) == (0, 1, 2)
    assert consts["HK_ABI_VERSION"] == 8   # additive: the ABI number stays


@pytest.mark.parametrize("fn", ["cast_rays", "cast_rays_device"])
def test_argument_refusals_on_a_null_context(fn):
    """Nothing here reaches a device: every refusal is decided from the arguments (flags, pointers, context - in that order)."""
    api = F.api()
    rays, hits = np.zeros(4, hk.RAY_DTYPE), np.full(4, 0xAB, np.uint8).repeat(48).view(hk.HIT_DTYPE)
    before = hits.tobytes()
    if fn == "cast_rays":
        pr, ph = C.cast(C.c_void_p(rays.ctypes.data), C.POINTER(F.HkRay)), C.cast(C.c_void_p(hits.ctypes.data), C.POINTER(F.HkRayHit))
    else:
        pr, ph = C.c_void_p(rays.ctypes.data), C.c_void_p(hits.ctypes.data)
    cases = [((None, pr, 4, 8, ph), "unknown ray query flag"), ((None, pr, 4, 0x80000000, ph), "unknown ray query flag"),
             ((None, pr, 4, F.RAYS_ANY | F.RAYS_ATTRIBUTES, ph), "HK_RAYS_ANY"), ((None, None, 4, 0, ph), "NULL rays or hits"),
             ((None, pr, 4, 0, None), "NULL rays or hits"), ((None, pr, 4, 0, ph), "ctx is NULL"), ((None, None, 0, 0, None), "ctx is NULL")]
    for args, text in cases:
        with pytest.raises(F.HikariError) as e:
            api.call(fn, *args)
        assert e.value.code == F.HK_E_INVALID and text in str(e.value), (args, str(e.value))
    assert hits.tobytes() == before


# ------------------------------------------------------------------------------------------------ Camera.ray_through
def _prepass_ids(scene, camera, lights=None):
    """(instance id per pixel or -1 for background) of the oracle's prepass: one frame without jitter (Taa::None)."""
    from oracle_lib import oracle_plugin

    p = oracle_plugin()
    p.set_scene(scene)
    s = hk.HikariSettings(indirect_bounces=0, denoise=False, temporal_reuse=False, indirect_spatial_reuse=False, taa=hk.Taa.NONE, upscale=hk.Upscale.SMAA_TU_1_0)
    p.render(camera, s, lights=lights, frame_number=1)
    p.engine.wait()
    depth = p.engine.read(F.BUF_POSITION)[:, :, 3]
    ids = np.floor(p.engine.read(F.BUF_INSTANCE_MATERIAL)[:, :, 0]).astype(np.int64)
    return np.where(depth > 0.0, ids, -1), p


@pytest.mark.parametrize("which", ["cornell_16x9", "yard_ortho"])
def test_ray_through_reproduces_the_prepass(which):
    """The ray through each pixel centre, traced by the reference's own walk, hits the instance the oracle's prepass stored in that
    pixel - everywhere except where the float64 caster says rounding decides (ray_ref: `ambiguous`), fewer than 5 % of the geometry
    pixels.  (The oracle alone satisfies this: the assertion below ran on it.)"""
    if which == "cornell_16x9":
        scene, cam, lights, tr = R.scene("cornell"), hk.cornell_camera(16, 9), None, R.triangles("cornell")
    else:
        import cases

        case = cases.make_case("yard_ortho")
        scene, lights = case.scene, case.lights
        cam = hk.Camera(case.camera.transform, 22, 16, ortho_height=case.camera.ortho_height)
        tr = R.Triangles(scene)
    ids, plugin = _prepass_ids(scene, cam, lights)
    h, w = ids.shape
    assert (h, w) == (cam.height, cam.width)
    od = [cam.ray_through((x + 0.5) / w, (y + 0.5) / h) for y in range(h) for x in range(w)]
    rays = hk.make_rays([o for o, _ in od], [d for _, d in od])
    assert np.allclose(np.linalg.norm(rays["direction"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    got = R.oracle_cast(plugin.engine, rays)
    ref = R.cast(tr, rays)
    want = ids.reshape(-1)
    traced = np.where(got["instance"] == R.NONE, -1, got["instance"].astype(np.int64))
    geometry = want >= 0
    assert geometry.sum() >= 0.25 * len(want), "the view shows too little geometry to test anything"
    wrong = (traced != want) & ~ref["ambiguous"]
    assert not wrong.any(), [(int(i % w), int(i // w), int(want[i]), int(traced[i])) for i in np.nonzero(wrong)[0][:8]]
    left_out = int((ref["ambiguous"] & geometry).sum())
    print(f"{which}: {int(geometry.sum())} geometry pixels, {left_out} left out as ambiguous")
    assert left_out < 0.05 * geometry.sum()
    if cam.ortho_height is not None:   # the origin lies on the near plane: all origins in one plane orthogonal to the direction
        o, d = rays["origin"].astype(np.float64), rays["direction"][0].astype(np.float64)
        assert np.ptp(o @ d) < 1e-4 and np.ptp(o, axis=0).max() > 1.0
    else:
        assert (rays["origin"] == np.array([0.0, 1.0, 4.0], np.float32)).all()


def test_rays_through_is_ray_through_for_arrays():
    import cases

    for cam in (hk.cornell_camera(31, 17), cases.make_case("yard_ortho").camera):
        u, v = np.array([0.0, 0.25, 0.5, 1.0, 0.7]), np.array([0.0, 0.5, 0.5, 1.0, 0.1])
        rays = cam.rays_through(u, v)
        assert rays.dtype == hk.RAY_DTYPE and (rays["exclude_instance"] == F.NO_INSTANCE).all() and (rays["max_distance"] == R.F32_MAX).all()
        for i in range(len(u)):
            o, d = cam.ray_through(u[i], v[i])
            assert np.allclose(rays["origin"][i], o, atol=1e-5) and np.allclose(rays["direction"][i], d, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("name", R.SCENES)
def test_the_reference_is_sane_on_the_inputs(name):
    """For every scene and set used on the GPU: the reference's walk and the float64 caster agree on hit / miss and on the identity
    for every ray float64 can decide; at least half the general rays hit; fewer than 2 % of them are ambiguous."""
    for set_name, rays in R.ray_sets(name).items():
        orc, ref = R.oracle_hits(name, set_name), R.float64_hits(name, set_name)
        clear = ~ref["ambiguous"]
        o_inst = np.where(orc["instance"] == R.NONE, -1, orc["instance"].astype(np.int64))
        o_prim = np.where(orc["primitive"] == R.NONE, -1, orc["primitive"].astype(np.int64))
        bad = clear & ((o_inst != ref["instance"]) | (o_prim != ref["primitive"]))
        assert not bad.any(), (name, set_name, [(int(i), int(o_inst[i]), int(ref["instance"][i]), ref["near"][i]) for i in np.nonzero(bad)[0][:5]])
        hit = clear & (ref["instance"] >= 0)
        scale = np.linalg.norm(rays["direction"].astype(np.float64), axis=1)
        err = np.abs(orc["distance"][hit].astype(np.float64) - ref["t"][hit]) * scale[hit]
        assert (err <= 1e-4 * np.maximum(1.0, ref["t"][hit] * scale[hit])).all(), (name, set_name, float(err.max()))
        miss = clear & (ref["instance"] < 0)
        assert (orc["distance"][miss] == rays["max_distance"][miss]).all()   # a miss holds max_distance
        print(f"{name}/{set_name}: {len(rays)} rays, {int((ref['instance'] >= 0).sum())} hit, {int(ref['ambiguous'].sum())} ambiguous")
        if set_name == "general":
            assert len(rays) == 1000 and (ref["instance"] >= 0).sum() >= 500
            assert ref["ambiguous"].sum() < 20
            assert np.isfinite(rays["max_distance"].astype(np.float64)).sum() and (rays["max_distance"] < R.F32_MAX).sum() == 333
            assert 50 <= (rays["exclude_instance"] != R.NONE).sum() <= 100
        if set_name == "ties":
            assert len(rays) >= 16 and ref["ambiguous"].mean() > 0.5   # the set is what it says: mostly two candidates within 1e-4


def test_the_invalid_set_has_one_ray_per_rule():
    rays, positions = R.invalid_rays("cornell")
    assert len(positions) == len(R.INVALID_RULES) == 10 and len(rays) == 128
    o, d, m = rays["origin"], rays["direction"], rays["max_distance"]
    bad = ~np.isfinite(o).all(axis=1) | ~np.isfinite(d).all(axis=1) | (d == 0).all(axis=1) | np.isnan(m) | (m < 0)
    assert sorted(np.nonzero(bad)[0]) == sorted(positions)
