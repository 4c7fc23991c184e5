"""Material edits on the host builder (hk_scene_builder_set_material): the next finish gives, byte for byte, what a builder that had
the new values from the start gives - the emitter radius, the emitter list, the alias tables and the light tree included.  And the
new entry points of the material / texture edits are declared in the header, bound in the ctypes table and in the generated Rust."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import SceneData
from bevy_hikari_amd.scenes import synthetic_scene
from conftest import ROOT

KW = dict(n_boxes=6, n_spheres=2, n_emitters=2, sphere_rings=4, sphere_segs=5)
# material ids of synthetic_scene: 0..7 plain, 8 and 9 the two emitters' own
PLAIN, EMITTERS = (1, 2, 3, 4, 5, 6, 7), (8, 9)


def copy_of(m):
    out = F.HkMaterial()
    C.memmove(C.byref(out), C.byref(m), C.sizeof(F.HkMaterial))
    return out


def edited(scene, edits):
    """{material id: HkMaterial} from {material id: callable(HkMaterial)} applied to copies of the scene's records."""
    out = {}
    for i, f in edits.items():
        m = copy_of(scene.materials[i])
        f(m)
        out[i] = m
    return out


def base_colour(m):
    m.base_color[:] = [0.05, 0.6, 0.3, 1.0]
    m.perceptual_roughness, m.metallic = 0.35, 1.0


def emitter_colour(m):
    m.emissive[:] = [0.3, 1.0, 0.55, 0.4]


def emitter_off(m):
    m.emissive[:] = [0.0, 0.0, 0.0, 1.0]


def emitter_on(m):
    m.emissive[:] = [0.9, 0.4, 0.2, 1.0]


def used_by_an_instance(scene, ids):
    used = {i.material for i in scene.instances}
    return [i for i in ids if i in used]


EDITS = {
    "base colour, roughness, metallic": lambda s: {used_by_an_instance(s, PLAIN)[0]: base_colour, 0: base_colour},
    "an emitter's colour and alpha": lambda s: {EMITTERS[1]: emitter_colour},
    "an emitter switched off": lambda s: {EMITTERS[0]: emitter_off},
    "a box material switched on": lambda s: {used_by_an_instance(s, PLAIN)[-1]: emitter_on},
    "all of them at once": lambda s: {used_by_an_instance(s, PLAIN)[0]: base_colour, EMITTERS[1]: emitter_colour, EMITTERS[0]: emitter_off,
                                      used_by_an_instance(s, PLAIN)[-1]: emitter_on},
}


def twin_with(materials):
    """synthetic_scene(**KW) built again, instance for instance, by a builder that has `materials` (a full list) from the start."""
    from bevy_hikari_amd.scenes import _box, _quad_strip, _sphere

    src, _ = synthetic_scene(**KW)
    b = hk.SceneBuilder()
    b.add_mesh(*_box())
    b.add_mesh(*_sphere(KW["sphere_rings"], KW["sphere_segs"]))
    qp, qn, quv = _quad_strip(4)
    b.add_mesh(qp, qn, quv, None, F.TOPOLOGY_TRIANGLE_STRIP)
    for m in materials:
        b.add_material(m)
    mesh_of = {}
    for k in range(3):   # (mesh ids of synthetic_scene: 0 box, 1 sphere, 2 quad strip)
        mi = src.builder.mesh_index(k)
        mesh_of[(mi.vertex, mi.primitive)] = k
    for inst in src.instances:
        b.add_instance(mesh_of[(inst.mesh.vertex, inst.mesh.primitive)], inst.material, np.ctypeslib.as_array(inst.model).copy())
    return b


def assert_same_scene(a: SceneData, b: SceneData, what):
    for name in SceneData.FIELDS:
        assert bytes(getattr(a, name)) == bytes(getattr(b, name)), f"{what}: {name} differs"
    assert np.asarray(a.previous_transforms).tobytes() == np.asarray(b.previous_transforms).tobytes(), f"{what}: previous transforms differ"


@pytest.mark.parametrize("what", list(EDITS))
def test_set_material_then_finish_equals_a_builder_that_had_the_values_from_the_start(what):
    scene, _ = synthetic_scene(**KW)
    new = edited(scene, EDITS[what](scene))
    n_emitters_before = len(scene.emissives)
    for i, m in new.items():
        scene.builder.set_material(i, m)
    got = scene.builder.finish()
    full = [new.get(i, scene.materials[i]) for i in range(len(scene.materials))]
    twin = twin_with(full)
    twin.finish()            # (the edited builder has been finished twice: so is the twin - the previous transforms are those of a finish)
    want = twin.finish()
    assert_same_scene(got, want, what)
    # the premises: the edit is visible where it should be
    if "off" in what or "on" in what:
        assert len(got.emissives) != n_emitters_before or "all" in what
    if "colour and alpha" in what:
        old = {e.instance: e.radius for e in scene.emissives}
        assert any(e.radius != old[e.instance] for e in got.emissives), "the emitter's radius must follow its colour"


def test_set_material_keeps_the_meshes_and_their_trees():
    scene, _ = synthetic_scene(**KW)
    scene.builder.set_material(EMITTERS[0], edited(scene, {EMITTERS[0]: emitter_off})[EMITTERS[0]])
    with pytest.raises(hk.HikariError) as err:    # un-finished at the instance level ...
        scene.builder.scene()
    assert err.value.code == F.HK_E_NOT_READY
    index = scene.builder.mesh_index(1)           # ... while the mesh level stays finished
    assert index.node_count > 0
    got = scene.builder.finish()
    for name in ("vertices", "primitives", "asset_nodes"):
        assert bytes(getattr(got, name)) == bytes(getattr(scene, name))


def test_set_material_refusals_leave_a_finished_builder_finished():
    scene, _ = synthetic_scene(**KW)
    b, api = scene.builder, F.api()
    m = copy_of(scene.materials[1])
    for args in ((b.h, len(scene.materials), C.byref(m)), (b.h, 0xFFFFFFFF, C.byref(m)), (b.h, 1, None), (None, 1, C.byref(m))):
        with pytest.raises(hk.HikariError) as err:
            api.call("scene_builder_set_material", *args)
        assert err.value.code == F.HK_E_INVALID
        assert_same_scene(b.scene(), scene, "after a refused set_material")   # (the getters still answer: the builder is finished)


def test_abi_version_is_unchanged():
    assert F.api().abi_version() == 8


NEW = ("hk_scene_builder_set_material", "hk_update_materials", "hk_multi_update_materials", "hk_update_texture", "hk_multi_update_texture")


def test_the_new_entry_points_are_declared_bound_and_generated():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hikari_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "hikari.hpp")).read()
    api = F.api()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in F.DECLARED_SYMBOLS and hasattr(api.dll, name), name
        assert re.search(r"pub fn " + name + r"\(", rust), name
        assert name + "(" in hpp, name
    assert callable(hk.SceneBuilder.set_material) and callable(hk.Engine.update_materials) and callable(hk.Engine.update_texture)
