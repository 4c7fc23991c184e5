"""hk_cast_rays / hk_cast_rays_device on the GPU (kernels_query.hip k_cast_rays) against the reference's own walk (orc_kat_trace) and the
float64 caster of tests/ray_ref.py: the three scenes that take the kernel's three stagings (one-level from LDS, two-level from LDS,
global memory with the wide or the skip-link walk), every ray set, closest and any-hit, the attributes, invalid rays, batch shapes,
the scene a query sees after updates, and that queries leave nothing behind in a frame."""
import os
import subprocess

import numpy as np
import pytest

import bevy_hikari_amd as hk
import ray_ref as R
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from cases import diff_buffers, make_case, product_default_traversal, snapshot
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXACT_MODE = {"cornell": ("reference", False), "small": ("reference", False), "large": ("reference", False)}
DEFAULT_MODE = {"cornell": ("one-level", False), "small": ("reference", False), "large": ("threaded", True)}
BITWISE = ("distance", "instance", "primitive", "barycentric")
_ENGINES = {}


def engine(name, exact=True):
    """One context per scene and mode for the whole module; asserts the walk it stands for, so that no case silently tests another."""
    key = (name, exact)
    if key not in _ENGINES:
        if exact:
            e = hk.Engine(device=0)          # the suite's default flags: HK_CTX_EXACT_TRAVERSAL
        else:
            with product_default_traversal():
                e = hk.Engine(device=0)
        e.upload_scene(R.scene(name))
        _ENGINES[key] = e
    e = _ENGINES[key]
    want = (EXACT_MODE if exact else DEFAULT_MODE)[name]
    assert (e.traversal_mode()[0], e.wide_walk()) == want, (name, exact, e.traversal_mode(), e.wide_walk())
    return e


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(got, want, fields, what, where=None):
    for f in fields:
        ne = (bits(got[f]) != bits(want[f])).reshape(len(got), -1).any(axis=1)
        if where is not None:
            ne &= where
        assert not ne.any(), (what, f, [(int(i), got[i], want[i]) for i in np.nonzero(ne)[0][:4]])


# ------------------------------------------------------------------------------------------------ 1. exact contexts, closest hit
@pytest.mark.parametrize("name", R.SCENES)
def test_exact_contexts_report_the_references_hit_bit_for_bit(name):
    e = engine(name)
    for set_name, rays in R.ray_sets(name).items():
        got, want = e.cast_rays(rays), R.oracle_hits(name, set_name)
        assert_same_bits(got, want, BITWISE, (name, set_name))
        assert ((got["status"] == F.RAY_HIT) == (got["instance"] != R.NONE)).all() and (got["status"] <= F.RAY_HIT).all()
        assert not got["material"].any() and not bits(got["uv"]).any() and not bits(got["normal"]).any()   # no HK_RAYS_ATTRIBUTES: zeros


# ------------------------------------------------------------------------------------------------ 2. batch shapes
@pytest.mark.parametrize("name,exact", [("small", True), ("cornell", False), ("large", False)])
def test_batch_shapes_and_the_device_entry_point(name, exact):
    torch = pytest.importorskip("torch")
    e = engine(name, exact)
    rays = R.general_rays(name)
    full = e.cast_rays(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32).copy()).cuda()
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        out = np.full(n + 1, 0xCD, np.uint8).repeat(48).view(hk.HIT_DTYPE)
        got = e.cast_rays(rays[:n], out=out[:n])
        assert got.tobytes() == full[:n].tobytes(), n
        assert out[n:].tobytes() == b"\xCD" * 48, n                        # the 48 bytes behind the last record keep their sentinel
        d_out = torch.full((n + 1, 48), 0xCD, dtype=torch.uint8, device="cuda")
        d_got = e.cast_rays(d_rays[:n], out=d_out[:n])
        host = d_out.cpu().numpy()
        assert (n == 0 or d_got.data_ptr() == d_out.data_ptr()) and host[:n].tobytes() == full[:n].tobytes(), n
        assert host[n:].tobytes() == b"\xCD" * 48, n


def test_more_rays_than_the_wide_walk_has_lanes():
    """The wide walk runs with at most as many lanes as the context's spill area serves (327 680 on 256 CUs) and a lane takes several
    rays; hk_cast_rays stages 262 144 rays per round trip.  700 001 rays pass both thresholds: every copy of the 1 000 rays answers
    as the 1 000 did."""
    e = engine("large", exact=False)
    rays = R.general_rays("large")
    base = e.cast_rays(rays)
    n = 700_001
    got = e.cast_rays(np.resize(rays, n))
    assert got.tobytes() == np.resize(base, n).tobytes()
    assert e.stats().wide_stack_lost == 0


# ------------------------------------------------------------------------------------------------ 3. any-hit
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", R.SCENES)
def test_any_hit_says_whether_the_reference_finds_a_hit(name, exact):
    e = engine(name, exact)
    for set_name, rays in R.ray_sets(name).items():
        got = e.cast_rays(rays, any_hit=True)
        want = np.where(R.oracle_hits(name, set_name)["instance"] != R.NONE, F.RAY_HIT, F.RAY_MISS)
        ne = got["status"] != want
        assert not ne.any(), (name, exact, set_name, [(int(i), rays[i]) for i in np.nonzero(ne)[0][:4]])


# ------------------------------------------------------------------------------------------------ 4. product default, closest hit
def _float64_distance(tr, ray, instance, primitive):
    c = np.nonzero((tr.instance == int(instance)) & (tr.primitive == int(primitive)))[0]
    assert len(c) == 1
    _u, _v, t, _det, _g = R._evaluate(tr, ray["origin"].astype(np.float64)[None], ray["direction"].astype(np.float64)[None])
    return float(t[0, c[0]])


def check_default_mode(name, got, set_name):
    """Where the identity equals the oracle's, distance and barycentrics are bit-equal.  An identity may differ only where the float64
    caster holds both candidates within 16 float32 ulps of each other - the combined rounding of one slab test and one triangle test
    (ties and box culls that depend on the visit order).  Returns the number of rays whose identity differs."""
    rays, want, tr = R.ray_sets(name)[set_name], R.oracle_hits(name, set_name), R.triangles(name)
    same = (got["instance"] == want["instance"]) & (got["primitive"] == want["primitive"])
    assert_same_bits(got, want, ("distance", "barycentric"), (name, set_name), where=same)
    assert ((got["status"] == F.RAY_HIT) == (got["instance"] != R.NONE)).all()
    for i in np.nonzero(~same)[0]:
        assert got["instance"][i] != R.NONE and want["instance"][i] != R.NONE, (name, set_name, int(i), rays[i], got[i], want[i])
        a = _float64_distance(tr, rays[i], got["instance"][i], got["primitive"][i])
        b = _float64_distance(tr, rays[i], want["instance"][i], want["primitive"][i])
        assert R.f32_ulps(a, b) <= 16.0, (name, set_name, int(i), rays[i], got[i], want[i], a, b)
    return int((~same).sum())


@pytest.mark.parametrize("name", R.SCENES)
def test_product_default_reports_the_references_hit_up_to_ties(name):
    e = engine(name, exact=False)
    e.reset_stats()
    for stackless in ((False, True) if name == "large" else (False,)):
        for set_name, rays in R.ray_sets(name).items():
            differing = check_default_mode(name, e.cast_rays(rays, stackless=stackless), set_name)
            print(f"{name}/{set_name} stackless={stackless}: {differing} of {len(rays)} identities differ from the reference's")
            if set_name == "general":
                assert differing <= 1   # at most 1 ray per 1 000; the expected count is 0
    assert e.stats().wide_stack_lost == 0


# ------------------------------------------------------------------------------------------------ 5. attributes
# The worst deviation from the float64 restatement measured on these sets (all three scenes, every set; MI355X): uv 7.215e-08 (Cornell),
# normal 1.375e-07 (the small yard).  The bound is twice that, rounded up to a whole float32 ulp of the largest component - both uv and
# unit normals reach 1.0, whose ulp is 2^-23 = 1.192e-07: 1.443e-07 -> 2 ulps, 2.750e-07 -> 3 ulps (DESIGN 2, and the table in DESIGN 4).
ULP_OF_ONE = 1.1920929e-07
UV_BOUND, NORMAL_BOUND = 2 * ULP_OF_ONE, 3 * ULP_OF_ONE


@pytest.mark.parametrize("name", R.SCENES)
def test_attributes_follow_hit_info(name):
    e, sc = engine(name), R.scene(name)
    worst_uv = worst_n = 0.0
    for set_name, rays in R.ray_sets(name).items():
        got = e.cast_rays(rays, attributes=True)
        assert_same_bits(got, R.oracle_hits(name, set_name), BITWISE, (name, set_name))   # the hit itself is the one without the flag
        mat, uv, nrm = R.hit_info_ref(sc, got)
        assert (got["material"] == mat).all()
        miss = got["instance"] == R.NONE
        assert not bits(got["uv"][miss]).any() and not bits(got["normal"][miss]).any()
        if (~miss).any():
            worst_uv = max(worst_uv, float(np.abs(got["uv"][~miss].astype(np.float64) - uv[~miss]).max()))
            worst_n = max(worst_n, float(np.abs(got["normal"][~miss].astype(np.float64) - nrm[~miss]).max()))
    print(f"{name}: worst deviation of uv {worst_uv:.3e} (bound {UV_BOUND:.3e}), of the normal {worst_n:.3e} (bound {NORMAL_BOUND:.3e})")
    assert worst_uv <= UV_BOUND and worst_n <= NORMAL_BOUND


# ------------------------------------------------------------------------------------------------ 6. invalid rays
@pytest.mark.parametrize("name,exact", [("cornell", True), ("cornell", False), ("large", False)])
def test_invalid_rays_are_refused_one_by_one(name, exact):
    e = engine(name, exact)
    rays, positions = R.invalid_rays(name)
    for kwargs in ({}, {"any_hit": True}, {"attributes": True}, {"stackless": True}):
        got = e.cast_rays(rays, **kwargs)                      # (returns: the launch is HK_OK)
        bad = np.zeros(len(rays), bool)
        bad[positions] = True
        assert (got["status"][bad] == F.RAY_INVALID).all() and (got["status"][~bad] != F.RAY_INVALID).all()
        assert (got["instance"][bad] == R.NONE).all() and (got["primitive"][bad] == R.NONE).all()
        assert (bits(got["distance"][bad]) == bits(rays["max_distance"][bad])).all()    # a miss holds max_distance, as given
        clean = e.cast_rays(R.general_rays(name)[:128], **kwargs)                        # the same 128 rays without the invalid ones
        if not kwargs.get("any_hit"):
            assert got[~bad].tobytes() == clean[~bad].tobytes()
        else:
            assert (got["status"][~bad] == clean["status"][~bad]).all()
    if exact:
        assert_same_bits(e.cast_rays(rays)[~bad], R.oracle_hits(name, "general")[:128][~bad], BITWISE, name)


# ------------------------------------------------------------------------------------------------ 7. the scene a query sees
SMALL = dict(n_boxes=10, n_spheres=3, n_emitters=2, sphere_rings=5, sphere_segs=6)


def test_queries_see_an_instance_update():
    sc, _sun = S.synthetic_scene(**SMALL)
    e = hk.Engine(device=0)
    e.upload_scene(sc)
    rays = R.plain_rays(R.Triangles(sc), 512, seed=5)
    before = e.cast_rays(rays)
    m = np.ctypeslib.as_array(sc.instances[4].model).copy()
    m[12:15] += np.array([0.7, 0.4, -0.9], np.float32)
    sc.builder.set_instance_transform(4, m)
    moved = sc.builder.finish()
    e.api.call("upload_scene_instances", e.ctx, sc.builder.h)
    after = e.cast_rays(rays)
    assert_same_bits(after, R.oracle_cast(R.oracle_engine(moved), rays), BITWISE, "moved")
    assert after.tobytes() != before.tobytes()


def test_queries_see_a_mesh_deformed_on_the_device():
    sc, _sun, meshes = S.deforming_scene("small")
    e = hk.Engine(device=0)
    e.upload_scene(sc)
    rays = R.plain_rays(R.Triangles(sc), 512, seed=6)
    before = e.cast_rays(rays)
    sphere = meshes["sphere"]
    p = S.pulsing_sphere(sphere["rest"], 2)
    e.update_mesh_vertices(sphere["index"], p)
    after = e.cast_rays(rays)
    sc.builder.set_mesh_vertices(sphere["id"], p, None)
    assert_same_bits(after, R.oracle_cast(R.oracle_engine(sc.builder.finish()), rays), BITWISE, "deformed")
    assert after.tobytes() != before.tobytes()


@pytest.mark.parametrize("exact", [True, False])
def test_queries_leave_nothing_behind_in_a_frame(exact):
    """The named case cornell_b2 rendered with batches of queries of every kind before and after each of its frames is byte for byte,
    in every buffer, the case rendered without them - in the suite's exact contexts and in product-default ones."""
    case = make_case("cornell_b2")
    rays = R.general_rays("cornell")

    def run(with_queries):
        if exact:
            p = hk.HikariPlugin(device=0)
        else:
            with product_default_traversal():
                p = hk.HikariPlugin(device=0)
        p.set_scene(case.scene)
        for n in case.frames:
            if with_queries:
                p.engine.cast_rays(rays[:300])
                p.engine.cast_rays(rays[300:600], any_hit=True)
            p.render(case.camera, case.settings, lights=case.lights, frame_number=n)
            if with_queries:
                p.engine.cast_rays(rays[600:], attributes=True)
        p.engine.wait()
        return snapshot(p)

    assert diff_buffers(run(True), run(False)) == {}


# ------------------------------------------------------------------------------------------------ 8. the C++ example
def test_the_cpp_example_picks_what_the_python_host_picks(tmp_path):
    """examples/cornell --pick 0.5 0.5: identity AND distance bits of Engine.cast_rays for cornell_camera(...).ray_through(0.5, 0.5) -
    include/hikari.hpp forms the ray with plugin.py's operations in plugin.py's order (doubles from the float32 uniforms), so the ray
    is the same bit for bit and so is the hit (both contexts are product-default ones).  The frames are the same with and without it."""
    exe = os.path.join(ROOT, "examples", "cornell")
    common = ["--size", "64", "48", "--frames", "2", "--bounces", "1", "--ratio", "1.0"]
    a = subprocess.run([exe] + common + ["--pick", "0.5", "0.5", "--raw", str(tmp_path / "a.bin")], capture_output=True, text=True, cwd=ROOT)
    b = subprocess.run([exe] + common + ["--raw", str(tmp_path / "b.bin")], capture_output=True, text=True, cwd=ROOT)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    lines = [l for l in a.stdout.splitlines() if l.startswith("pick ")]
    assert len(lines) == 1 and not [l for l in b.stdout.splitlines() if l.startswith("pick ")]
    _, inst, prim, dist = lines[0].split()
    o, d = hk.cornell_camera(64, 48).ray_through(0.5, 0.5)
    want = engine("cornell", exact=False).cast_rays(hk.make_rays([o], [d]))[0]
    assert want["status"] == F.RAY_HIT
    assert (int(inst), int(prim)) == (int(want["instance"]), int(want["primitive"]))
    assert np.float32(dist).view(np.uint32) == want["distance"].view(np.uint32), (dist, float(want["distance"]))
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
