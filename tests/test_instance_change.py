"""hk_change_scene_instances without a GPU: the origin bookkeeping of the Python builder wrapper, the layout rule the device call relies on
(a builder edited in place lays its instance level out byte for byte like a builder that had the final set from the start), and the
presence of the entry points in every binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scene_edit_model as M
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.plugin import SceneBuilder
from conftest import ROOT

BASE = "two_slot"


def edited_and_direct(seed, n_edits):
    """(a base builder edited in place by a seeded sequence of instance adds, removes and re-materials, a builder given the final set from
    the start, the tokens of the final instances: an int for an instance of the base scene, None for a new one)"""
    rng = np.random.default_rng(seed)
    d = M.base_description(BASE)
    names = [n for n, _ in d["meshes"]]
    b = M.base_builder(BASE)
    b.take_origins()   # (a context took the base scene)
    final = [dict(token=k, mesh=names.index(n), material=m, pose=M.instance_pose(BASE, p)) for k, (n, m, p) in enumerate(d["instances"])]
    for step in range(n_edits):
        kind = rng.choice(["add", "remove", "material"]) if len(final) > 1 else "add"
        if kind == "add":
            inst = dict(token=None, mesh=int(rng.integers(0, len(names))), material=int(rng.integers(0, len(d["materials"]))), pose=M.pose(BASE, 1000 * seed + step))
            b.add_instance(inst["mesh"], inst["material"], inst["pose"])
            final.append(inst)
        elif kind == "remove":
            k = int(rng.integers(0, len(final)))
            b.remove_instance(k)
            del final[k]
        else:
            k, mat = int(rng.integers(0, len(final))), int(rng.integers(0, len(d["materials"])))
            b.set_instance_material(k, mat)
            final[k]["material"] = mat
    direct = SceneBuilder()
    for k in range(len(d["materials"])):
        direct.add_material(M.material(BASE, k, 0))
    for name in names:
        M.add_pool_mesh(direct, BASE, name, "host")
    for inst in final:
        direct.add_instance(inst["mesh"], inst["material"], inst["pose"])
    return b, direct, [inst["token"] for inst in final]


@pytest.mark.parametrize("seed", range(6))
def test_the_wrapper_keeps_the_origin_of_every_instance(seed):
    b, _, tokens = edited_and_direct(seed, 25)
    want = [F.INSTANCE_NEW if t is None else t for t in tokens]
    assert list(b.origins) == want
    survivors = [o for o in b.origins if o != F.INSTANCE_NEW]
    assert len(set(survivors)) == len(survivors)
    taken = b.take_origins()
    assert taken.dtype == np.uint32 and taken.tolist() == want
    assert list(b.origins) == list(range(len(tokens))), "a consumed list is the identity: every instance is its own origin"
    b.add_instance(0, 0, M.pose(BASE, 7))
    b.remove_instance(0)
    assert list(b.origins) == list(range(1, len(tokens))) + [F.INSTANCE_NEW]


@pytest.mark.parametrize("seed", range(4))
def test_a_builder_edited_in_place_lays_out_what_a_builder_with_the_final_set_does(seed):
    """the host layout of hk_change_scene_instances: counts, offsets, the emitter list's order and the alias slices depend on the final
    set alone, not on the edits that led to it"""
    b, direct, _ = edited_and_direct(seed, 12)
    a, w = b.finish(build_trees=False), direct.finish(build_trees=False)
    for name in ("instances", "instance_nodes", "emissives", "emissive_nodes", "alias_table", "materials"):
        assert bytes(getattr(a, name)) == bytes(getattr(w, name)), f"seed {seed}: {name} differ"
    assert len(a.emissives) >= 1 or not any(M.base_description(BASE)["materials"][i.material][1] != (0, 0, 0) for i in a.instances)


def test_the_entry_points_are_in_every_binding():
    header = open(os.path.join(ROOT, "include", "hikari_hip.h")).read()
    debug = open(os.path.join(ROOT, "include", "hikari_hip_debug.h")).read()
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    cpp = open(os.path.join(ROOT, "include", "hikari.hpp")).read()
    assert re.search(r"#define HK_INSTANCE_NEW 0xFFFFFFFFu", header)
    assert re.search(r"int hk_change_scene_instances\(hk_ctx\* ctx, hk_scene_builder\* b, const uint32_t\* origins, uint32_t n, uint32_t tree_mode\);", header)
    assert re.search(r"int hk_multi_change_scene_instances\(hk_multi\* m, hk_scene_builder\* b, const uint32_t\* origins, uint32_t n, uint32_t tree_mode\);", header)
    assert re.search(r"int hk_debug_last_instance_change\(hk_ctx\* ctx, uint32_t out\[4\]\);", debug)
    assert re.search(r"pub fn hk_change_scene_instances\(ctx: \*mut HkCtx, b: \*mut HkSceneBuilder, origins: \*const u32, n: u32, tree_mode: u32\) -> i32;", rust)
    assert re.search(r"pub fn hk_multi_change_scene_instances\(m: \*mut HkMulti, b: \*mut HkSceneBuilder, origins: \*const u32, n: u32, tree_mode: u32\) -> i32;", rust)
    assert re.search(r"pub const HK_INSTANCE_NEW: u32 = 4294967295;", rust)
    assert cpp.count("hk_change_scene_instances(") == 1 and cpp.count("hk_multi_change_scene_instances(") == 1
    assert F.INSTANCE_NEW == 0xFFFFFFFF
    api = F.api()
    for name in ("hk_change_scene_instances", "hk_multi_change_scene_instances", "hk_debug_last_instance_change"):
        assert hasattr(api.dll, name), name
    assert "hk_debug_last_instance_change" in F.DECLARED_DEBUG_SYMBOLS
    assert api.raw("change_scene_instances").argtypes[2:] == [C.POINTER(F.u32), F.u32, F.u32]


def test_the_call_refuses_what_it_can_without_a_device():
    """NULL arguments come back as HK_E_INVALID before anything touches a device"""
    b = M.base_builder(BASE)
    origins = (F.u32 * 8)(*range(8))
    assert F.api().raw("change_scene_instances")(None, b.h, origins, 5, F.TREE_SAH) == F.HK_E_INVALID
