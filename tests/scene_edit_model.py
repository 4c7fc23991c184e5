"""A model of the scene-edit calls of include/hikari_hip.h: seeded sequences of edits on a loaded scene, the states they lead through, and the
end state a freshly loaded twin needs.  Host only: nothing here touches a GPU (test_scene_edit_sequences.py runs it without one,
test_scene_edit_sequences_gpu.py drives contexts with it).

An op is a small record: a kind, plain arguments (names of pool meshes, instance positions, material ids) and a seed for its data.  Meshes
are named by their pool name ("s7": the soup of 7 triangles of tests/test_remove_meshes_gpu.py, "cloth", "cylinder", "sphere"), never by
id: ids and records move with every removal, and following them is what the model is for.

Families and kinds
  mesh_set      add_meshes (one to three, deferred or host-built; instances follow through update_instances_on_device where that call is
                accepted), remove_meshes (one to three; their instances go first)
  instance_set  add_instance, remove_instance, set_instance_material - each followed by update_instances_on_device
  poses         refit_instances (poses set on the builder), set_instance_transforms (a device tensor; all instances or an `ids` subset)
  geometry      update_mesh_vertices, deform_meshes (host items: vertices, skin, morph, morph_skin), deform_meshes_device (the same items from
                device tensors; vertices items may ask for recomputed normals), set_mesh_skin, set_mesh_morph_targets
  trees         rebuild_mesh_tree(HK_TREE_SAH), rebuild_trees(HK_TREE_SAH)
  appearance    set_material (+ update_materials), update_texture (host), update_textures (a rectangle from a device tensor: uint8, float16
                or float32)
  observers     frame (enqueued, not waited for), cast_rays (256 rays), read_mesh_nodes

Legality table.  The table below, not the library, decides what the generator emits and what a deliberate refusal must return.  Quotes are
from include/hikari_hip.h.

  family        accepted                                              refused (row: code)
  ------------  ----------------------------------------------------  -------------------------------------------------------------------
  mesh_set      two slots: "Accepted in every state hk_add_meshes is  one_slot_add_stale: HK_E_NOT_READY - "A scene walked from the LDS
                accepted in (mirrors stale or fresh)"; hk_add_meshes  copy (one slot) ... HK_E_NOT_READY when the mirrors are stale, as any
                "is accepted after hk_refit_scene_instances,          re-layout".  one_slot_remove_stale: HK_E_NOT_READY - "HK_E_NOT_READY
                hk_rebuild_scene_trees, hk_update_materials,          with NOTHING changed when the mirrors are stale or a mesh was
                hk_update_mesh_vertices, hk_skin_mesh and             deformed".  remove_instanced: HK_E_INVALID - "an uploaded instance
                hk_rebuild_mesh_tree".  One slot: while the mirrors   whose mesh lies inside an extent" (both scenes, every state).
                are fresh and no mesh was deformed.
  instance_set  until the first deformation and the first device      instances_after_deformation: HK_E_NOT_READY - "hk_update_scene_
                pose call                                             instances is still refused after a deformation".
                                                                      instances_after_device_poses: HK_E_NOT_READY - "What would diff
                                                                      against or lay out from them is refused with HK_E_NOT_READY:
                                                                      hk_refit_scene_instances, hk_update_scene_instances".
  poses         set_instance_transforms always; refit_instances       refit_after_device_poses: HK_E_NOT_READY (the quote above).
                until the first device pose call ("hk_rebuild_scene_
                trees and hk_refit_scene_instances work from the
                device's current boxes" after a deformation)
  geometry      a mesh an uploaded instance carries ("it must equal   skin_without_skin: HK_E_INVALID - "no skin set".
                an uploaded instance's record"); skin / morph items   morph_without_set: HK_E_INVALID - "no morph set for the mesh".
                once the mesh has its skin / morph set
  trees         always (rebuild_mesh_tree: a mesh an instance
                carries)
  appearance    update_materials case A always ("Case A works after
                refits, device tree rebuilds and mesh deformations");
                the model never switches an emitter on or off.
                hk_update_texture "Works whatever was changed on the
                device before"; hk_update_textures_device alike.
  observers     always

What makes the mirrors stale, as the model counts it: refit_instances, set_instance_transforms, rebuild_trees, update_instances_on_device
of a scene with two instances or more (it ends in hk_rebuild_scene_trees), every deformation and rebuild_mesh_tree, and an update_materials
that changed an emissive colour ("The host copies become stale ... only if an emitter record changed" - the model counts that as `maybe`: it
neither emits a one-slot mesh-set op nor a deliberate refusal of one in that state).  Nothing in the vocabulary makes them fresh again
(hk_upload_scene would, and drops every skin and morph set: it is not an edit of a loaded scene).

Ordering rules the executor follows: "one call per builder finish, in order" - a remove_meshes op removes its meshes from the builder back
to front, makes one call and finishes; an add_meshes op adds, finishes and makes one call.  Every op leaves the live builder finished at the
mesh level, with no deferred mesh pending and no extent handed out and not yet used: the builder's finished and pending marks and the
extents removed since its last finish are the same in front of every op, so the state carries no field for them - a field that never varies
decides nothing in the table.
"""
import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S

FAMILY = dict(add_meshes="mesh_set", remove_meshes="mesh_set",
              add_instance="instance_set", remove_instance="instance_set", set_instance_material="instance_set",
              refit_instances="poses", set_instance_transforms="poses",
              update_mesh_vertices="geometry", deform_meshes="geometry", deform_meshes_device="geometry", set_mesh_skin="geometry", set_mesh_morph_targets="geometry",
              rebuild_mesh_tree="trees", rebuild_trees="trees",
              set_material="appearance", update_texture="appearance", update_textures="appearance",
              frame="observers", cast_rays="observers", read_mesh_nodes="observers")
KINDS = tuple(FAMILY)
FAMILIES = ("mesh_set", "instance_set", "poses", "geometry", "trees", "appearance", "observers")
#: refusal row -> the code the call must return
REFUSALS = dict(one_slot_add_stale=F.HK_E_NOT_READY, one_slot_remove_stale=F.HK_E_NOT_READY, remove_instanced=F.HK_E_INVALID,
                instances_after_deformation=F.HK_E_NOT_READY, instances_after_device_poses=F.HK_E_NOT_READY, refit_after_device_poses=F.HK_E_NOT_READY,
                skin_without_skin=F.HK_E_INVALID, morph_without_set=F.HK_E_INVALID)
#: the rows a base scene can reach
REFUSAL_ROWS = dict(two_slot=tuple(r for r in REFUSALS if not r.startswith("one_slot")), one_slot=tuple(REFUSALS))
BASES = ("two_slot", "one_slot")
REFUSAL_PROBABILITY = 0.12
DEFORMING = ("update_mesh_vertices", "deform_meshes", "deform_meshes_device", "rebuild_mesh_tree")   # what sets `deformed`
LDS_SCENE_BYTES = 32768
N_MORPH_TARGETS = 3


class Op:
    __slots__ = ("kind", "args", "seed", "refuse")

    def __init__(self, kind, args=None, seed=0, refuse=None):
        self.kind, self.args, self.seed, self.refuse = kind, dict(args or {}), int(seed), refuse

    @property
    def family(self):
        return FAMILY[self.kind]

    def meshes(self):
        """the pool names the op touches (empty: a scene-wide op)"""
        a = self.args
        if self.kind == "add_meshes":
            return [m for m, _ in a["meshes"]]
        if self.kind == "remove_meshes":
            return list(a["meshes"])
        if self.kind in ("deform_meshes", "deform_meshes_device"):
            return [it[1] for it in a["items"]]
        if "mesh" in a:
            return [a["mesh"]]
        return []

    def key(self):
        return (self.kind, repr(sorted(self.args.items())), self.seed, self.refuse)

    def __repr__(self):
        return f"Op({self.kind!r}, {self.args!r}, seed={self.seed}" + (f", refuse={self.refuse!r})" if self.refuse else ")")


# ------------------------------------------------------------------------------------------------------------------------- the pool
_POOL = {}
SOUPS = {"s7": 0, "s1100": 1, "s1": 2, "s2": 3, "s3": 4, "s40": 5, "s300": 6, "s1025": 7}   # name -> mesh k of tests/test_remove_meshes_gpu.py


def pool(base, name):
    """dict(positions, normals, uvs, indices[, joints, weights]) of a pool mesh.  The soups are those of test_remove_meshes_gpu.mesh_data (1, 2,
    3, 7, 40 - with three vertices no triangle names - 300, 1 025 and the base's 1 100 triangles); the deformables are sized by the base scene:
    the one-slot scene must stay inside the LDS copy whatever is added to it."""
    key = (base if name in ("cloth", "cylinder", "sphere") else "", name)
    if key not in _POOL:
        if name in SOUPS:
            from test_remove_meshes_gpu import mesh_data

            p, n, uv, i = mesh_data(SOUPS[name])
            _POOL[key] = dict(positions=p, normals=n, uvs=uv, indices=i)
        elif name[0] == "c" and name[1:].isdigit():   # a Cornell mesh
            import json
            import os

            from bevy_hikari_amd.plugin import ASSETS

            with open(os.path.join(ASSETS, "cornell.json")) as f:
                m = json.load(f)["meshes"][int(name[1:])]
            _POOL[key] = dict(positions=np.asarray(m["positions"], np.float32).reshape(-1, 3), normals=np.asarray(m["normals"], np.float32).reshape(-1, 3),
                              uvs=np.asarray(m["uvs"], np.float32).reshape(-1, 2), indices=np.asarray(m["indices"], np.uint32).reshape(-1))
        else:
            big = base == "two_slot"
            if name == "cloth":
                p, n, uv, i = S.cloth_grid(6, 5, size=1.5) if big else S.cloth_grid(2, 2, size=1.5)
                _POOL[key] = dict(positions=p, normals=n, uvs=uv, indices=i)
            elif name == "cylinder":
                p, n, uv, i, ji, jw = S.bending_cylinder() if big else S.bending_cylinder(rings=2, segs=3)
                _POOL[key] = dict(positions=p, normals=n, uvs=uv, indices=i, joints=ji, weights=jw)
            elif name == "sphere":
                p, n, uv, i = S._sphere(5, 7) if big else S._sphere(2, 3)
                _POOL[key] = dict(positions=p, normals=n, uvs=uv, indices=i)
            else:
                raise KeyError(name)
    return _POOL[key]


def n_triangles(base, name):
    return len(pool(base, name)["indices"]) // 3


def n_vertices(base, name):
    return len(pool(base, name)["positions"])


DEFORMABLE = ("cloth", "cylinder", "sphere")
SKINNABLE = ("cylinder",)
MORPHABLE = ("sphere", "cylinder")   # (the cylinder with both a skin and a morph set takes morph_skin items)
ADDABLE = dict(two_slot=("s1", "s2", "s3", "s300", "s1025", "s7", "s40", "cloth", "cylinder", "sphere"), one_slot=("s1", "s2", "s3", "s7", "cloth", "cylinder", "sphere"))


# ------------------------------------------------------------------------------------------------------------------------- op data
def pose(base, seed):
    """the 16 floats (column-major) of pose `seed`"""
    rng = np.random.default_rng(50_000 + seed)
    if base == "two_slot":
        t, s = rng.uniform((-1.2, 0.2, -0.6), (1.2, 1.6, 0.6)), rng.uniform(0.4, 0.8, 3)
    else:
        t, s = rng.uniform((-0.6, 0.3, -0.5), (0.6, 1.5, 0.5)), rng.uniform(0.15, 0.35, 3)
    return S._trs(tuple(t), tuple(rng.uniform(-1.0, 1.0, 3)), tuple(s))


def material(base, mid, version):
    """material `mid` of the base scene in its `version` (0: as loaded).  Emissive materials stay emissive, the others dark: every
    update_materials is the call's case A."""
    recs = base_description(base)["materials"]
    base_color, emissive, rough, texture = recs[mid]
    if version:
        rng = np.random.default_rng(60_000 + 100 * version + mid)
        base_color = tuple(rng.uniform(0.1, 0.9, 3)) + (1.0,)
        rough = float(rng.uniform(0.2, 0.9))
        if any(emissive):
            emissive = tuple(float(c) for c in np.asarray(emissive) * rng.uniform(0.5, 1.5))
    m = S.standard_material(base_color, emissive, rough, 0.0, 0.5)
    if texture is not None:
        m.base_color_texture = texture
    return m


def base_textures():
    """two small textures: 16 x 16 sRGB sampled at the nearest texel, 12 x 8 linear-format bilinear"""
    rng = np.random.default_rng(70_000)
    return [dict(rgba=rng.integers(0, 256, (16, 16, 4), dtype=np.uint8), srgb=True, linear=False),
            dict(rgba=rng.integers(0, 256, (8, 12, 4), dtype=np.uint8), srgb=False, linear=True)]


def texture_image(index, seed):
    """the whole image an update_texture op uploads (sampler unchanged)"""
    t = base_textures()[index]
    rng = np.random.default_rng(71_000 + seed)
    return dict(rgba=rng.integers(0, 256, t["rgba"].shape, dtype=np.uint8), srgb=t["srgb"], linear=t["linear"])


TEXEL_TYPES = ("uint8", "float16", "float32")


def texture_rectangle(args, seed):
    """the [h][w][4] source array of an update_textures op, of the op's type (floats: the encoded value in [0, 1])"""
    rng = np.random.default_rng(72_000 + seed)
    shape = (args["h"], args["w"], 4)
    if args["dtype"] == "uint8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.uniform(0.0, 1.0, shape).astype(args["dtype"])


def vertex_data(base, name, seed, with_normals):
    """(positions, normals or None) of a vertices item: the cloth waves, every other mesh is scaled and jittered"""
    d = pool(base, name)
    rng = np.random.default_rng(80_000 + seed)
    if name == "cloth":
        p, n = S.waving_cloth(d["positions"], seed % 23, amplitude=0.12)
    else:
        p = (d["positions"] * np.float32(1.0 + 0.2 * rng.uniform(-1.0, 1.0)) + rng.normal(0.0, 0.01, d["positions"].shape)).astype(np.float32)
        n = rng.normal(size=p.shape)
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return p, (n if with_normals else None)


def morph_set(base, name):
    """(base positions, base normals, position deltas, normal deltas) of the mesh's morph set"""
    d = pool(base, name)
    rng = np.random.default_rng(81_000 + len(name))
    dp = rng.normal(0.0, 0.05, (N_MORPH_TARGETS,) + d["positions"].shape).astype(np.float32)
    dn = rng.normal(0.0, 0.1, (N_MORPH_TARGETS,) + d["positions"].shape).astype(np.float32)
    return d["positions"], d["normals"], dp, dn


def morph_weights(seed):
    return S.morph_weights(N_MORPH_TARGETS, seed % 11, mode="wave")


def joints(seed):
    return S.bend_joints(seed % 13)


def item_result(base, item):
    """(positions, normals or None: kept) a deformation item leaves, by the host twins of the device contracts: hk_morph_vertices for the
    morph arithmetic, the float32 restatement of the skinning contract (scenes.skin_reference)"""
    from bevy_hikari_amd.plugin import morph_vertices

    kind, name, seed = item[0], item[1], item[2]
    d = pool(base, name)
    if kind == "vertices":
        return vertex_data(base, name, seed, item[3] == "normals")
    if kind == "skin":
        return S.skin_reference(d["positions"], d["normals"], d["joints"], d["weights"], joints(seed))
    if kind == "morph":
        return morph_vertices(*morph_set(base, name), morph_weights(seed))
    if kind == "morph_skin":
        p, n = morph_vertices(*morph_set(base, name), morph_weights(seed + 1))
        return S.skin_reference(p, n, d["joints"], d["weights"], joints(seed))
    raise KeyError(kind)


def ray_batch(base, seed, n=256):
    """origins and directions of a cast_rays op"""
    rng = np.random.default_rng(90_000 + seed)
    lo, hi = ((-3.0, -1.0, -3.0), (3.0, 3.0, 3.0)) if base == "two_slot" else ((-0.9, 0.1, -0.9), (0.9, 1.9, 3.5))
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    target = rng.uniform((-1.0, 0.0, -1.0), (1.0, 1.8, 1.0), (n, 3)).astype(np.float32)
    return o, target - o


# ------------------------------------------------------------------------------------------------------------------------- base scenes
def base_description(base):
    """dict(meshes=[(name, pinned)], instances=[(mesh name, material, pose or None: see instance_pose)], materials=[(base colour, emissive,
    roughness, texture or None)]) of a base scene.
      two_slot  held beyond the LDS copy by the 1 100-triangle soup (tests/test_remove_meshes_gpu.py); the soups of 7 and 40 triangles, the
                cloth, the bending cylinder and the sphere (glowing: its deformations move an emitter); the mesh of 40 has no instance
      one_slot  Cornell (its eight meshes pinned) plus the soups of 7, 3 and 2 triangles and small deformables; the soups of 3 and 2 have
                no instance, so they can leave while the mirrors are fresh"""
    grey, glow = ((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, None), ((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, None)
    textured, green = ((1.0, 1.0, 1.0, 1.0), (0, 0, 0), 0.8, 0), ((0.2, 0.6, 0.3, 1.0), (0, 0, 0), 0.6, 1)
    if base == "two_slot":
        return dict(meshes=[("s1100", True), ("s7", False), ("cloth", False), ("cylinder", False), ("sphere", False), ("s40", False)],
                    instances=[("s1100", 0, 1), ("s7", 3, 2), ("cloth", 1, 3), ("cylinder", 0, 4), ("sphere", 2, 5)],
                    materials=[grey, textured, glow, green])
    import json
    import os

    from bevy_hikari_amd.plugin import ASSETS

    with open(os.path.join(ASSETS, "cornell.json")) as f:
        j = json.load(f)
    mats = [(tuple(m["base_color_factor"]), tuple(m["emissive_factor"]), m["roughness_factor"], None) for m in j["materials"]]
    assert all(m["metallic_factor"] == 0.0 for m in j["materials"])
    meshes = [(f"c{k}", True) for k in range(len(j["meshes"]))]
    inst = [(f"c{i['mesh']}", j["meshes"][i["mesh"]]["material"], tuple(i["transform"]) if not isinstance(i["transform"][0], list) else tuple(np.asarray(i["transform"]).reshape(-1)))
            for i in j["instances"]]
    n = len(mats)
    return dict(meshes=meshes + [("s7", False), ("cloth", False), ("cylinder", False), ("sphere", False), ("s3", False), ("s2", False)],
                instances=inst + [("s7", n + 1, 2), ("cloth", n, 3), ("cylinder", 0, 4), ("sphere", n + 2, 5)],
                materials=mats + [textured, green, glow])


def instance_pose(base, p):
    """an instance's 16 floats: pose seeds are ints, Cornell's own transforms are kept as tuples"""
    return np.asarray(p, np.float32).reshape(-1) if isinstance(p, tuple) else pose(base, p)


# ------------------------------------------------------------------------------------------------------------------------- the state
class State:
    """What the legality table reads, and what the twin needs.  apply(op) is the only transition; refused ops change nothing."""

    def __init__(self, base):
        d = base_description(base)
        self.base = base
        self.slots = 2 if base == "two_slot" else 1
        self.meshes = [dict(name=n, how="host", pinned=p) for n, p in d["meshes"]]            # id order
        self.instances = [dict(mesh=m, material=mat, pose=p) for m, mat, p in d["instances"]]  # id order
        self.materials = [0] * len(d["materials"])                                             # version per material
        self.textures = [t["rgba"].copy() for t in base_textures()]
        self.stale = False          # the mirrors are stale for certain
        self.stale_maybe = False    # ... or may be (an emissive colour changed)
        self.deformed = False       # a mesh was deformed (or its tree rebuilt) on the device
        self.device_poses = False   # poses were set from device memory
        self.skins, self.morphs, self.rebuilt = [], [], []
        # meshes the scene was loaded with that no instance has carried yet: an upload derives the final form of a mesh's range when its first
        # instance arrives (one more host layout of the mesh level); what hk_add_meshes appends is in final form at once
        self.raw = [m["name"] for m in self.meshes if not self.instances_of(m["name"])]
        self.history = {}           # name -> the geometry and tree ops that named the mesh, in order (entries of item_result's form)
        self.recent = []            # the meshes recent ops touched, latest last
        self.frames = 0

    # -- queries
    def names(self):
        return [m["name"] for m in self.meshes]

    def mesh_id(self, name):
        return self.names().index(name)

    def instanced(self):
        return sorted({i["mesh"] for i in self.instances})

    def instances_of(self, name):
        return [k for k, i in enumerate(self.instances) if i["mesh"] == name]

    def lds_estimate(self):
        """the library's own estimate of the scene's size (scene_layout.hip wants_threaded), generously rounded up"""
        nt = sum(n_triangles(self.base, m["name"]) for m in self.meshes)
        nv = sum(n_vertices(self.base, m["name"]) for m in self.meshes)
        ni = len(self.instances)
        return (3 * nt) * 32 + nt * 48 + nv * 24 + 2 * ni * 32 + ni * 208 + len(self.materials) * 64 + 64 * 40 + nt * 8

    def instance_ops_legal(self):
        return not self.deformed and not self.device_poses

    def mesh_set_legal(self):
        return self.slots == 2 or not (self.stale or self.stale_maybe or self.deformed)

    def refusal_row(self, op):
        """the row of the table that refuses `op` in this state, or None: accepted"""
        k = op.kind
        if k in ("add_instance", "remove_instance", "set_instance_material"):
            return "instances_after_deformation" if self.deformed else "instances_after_device_poses" if self.device_poses else None
        if k == "refit_instances":
            return "refit_after_device_poses" if self.device_poses else None
        if k == "add_meshes":
            return None if self.slots == 2 or not (self.stale or self.deformed) else "one_slot_add_stale"
        if k == "remove_meshes":
            if any(self.instances_of(m) for m in op.args["meshes"]) and not op.args.get("drop_instances"):
                return "remove_instanced"
            return None if self.slots == 2 or not (self.stale or self.deformed) else "one_slot_remove_stale"
        if k in ("deform_meshes", "deform_meshes_device"):
            for it in op.args["items"]:
                if it[0] in ("skin", "morph_skin") and it[1] not in self.skins:
                    return "skin_without_skin"
                if it[0] in ("morph", "morph_skin") and it[1] not in self.morphs:
                    return "morph_without_set"
        return None

    # -- the transition
    def touch(self, names):
        for n in names:
            if n in self.recent:
                self.recent.remove(n)
            self.recent.append(n)
        del self.recent[:-4]

    def apply(self, op):
        if op.refuse:
            assert self.refusal_row(op) == op.refuse, (op, self.refusal_row(op))
            return
        assert self.refusal_row(op) is None, (op, self.refusal_row(op))
        k, a = op.kind, op.args
        many = len(self.instances) >= 2
        if k == "add_meshes":
            for name, how in a["meshes"]:
                assert name not in self.names()
                self.meshes.append(dict(name=name, how=how, pinned=False))
            if a["instances"]:
                assert self.instance_ops_legal()
                for name, mat, p in a["instances"]:
                    self.instances.append(dict(mesh=name, material=mat, pose=p))
                self.stale = self.stale or len(self.instances) >= 2
        elif k == "remove_meshes":
            drop = sorted(a.get("drop_instances", []), reverse=True)
            if drop:
                assert self.instance_ops_legal()
                for i in drop:
                    assert self.instances[i]["mesh"] in a["meshes"]
                    del self.instances[i]
                self.stale = self.stale or len(self.instances) >= 2
            for name in a["meshes"]:
                m = self.meshes[self.mesh_id(name)]
                assert not m["pinned"] and not self.instances_of(name)
                self.meshes.remove(m)
                for group in (self.skins, self.morphs, self.rebuilt):
                    if name in group:
                        group.remove(name)
                self.history.pop(name, None)
        elif k == "add_instance":
            self.instances.append(dict(mesh=a["mesh"], material=a["material"], pose=op.seed))
            self.stale = self.stale or len(self.instances) >= 2
        elif k == "remove_instance":
            del self.instances[a["instance"]]
            self.stale = self.stale or len(self.instances) >= 2
        elif k == "set_instance_material":
            self.instances[a["instance"]]["material"] = a["material"]
            self.stale = self.stale or many
        elif k == "refit_instances":
            for i, p in a["poses"]:
                self.instances[i]["pose"] = p
            self.stale = True
        elif k == "set_instance_transforms":
            for i, p in a["poses"]:
                self.instances[i]["pose"] = p
            self.stale = self.device_poses = True
        elif k == "update_mesh_vertices":
            self.history.setdefault(a["mesh"], []).append(("vertices", a["mesh"], op.seed, a["normals"]))
            self.stale = self.deformed = True
        elif k in ("deform_meshes", "deform_meshes_device"):
            for it in a["items"]:
                self.history.setdefault(it[1], []).append(tuple(it))
            self.stale = self.deformed = True
        elif k == "set_mesh_skin":
            self.skins.append(a["mesh"])
            self.history.setdefault(a["mesh"], []).append(("set_skin", a["mesh"]))
        elif k == "set_mesh_morph_targets":
            self.morphs.append(a["mesh"])
            self.history.setdefault(a["mesh"], []).append(("set_morph", a["mesh"]))
        elif k == "rebuild_mesh_tree":
            if a["mesh"] not in self.rebuilt:
                self.rebuilt.append(a["mesh"])
            self.history.setdefault(a["mesh"], []).append(("rebuild", a["mesh"]))
            self.stale = self.deformed = True
        elif k == "rebuild_trees":
            self.stale = True
        elif k == "set_material":
            self.materials[a["material"]] = a["version"]
            if any(base_description(self.base)["materials"][a["material"]][1]):
                self.stale_maybe = True
        elif k == "update_texture":
            self.textures[a["texture"]] = texture_image(a["texture"], op.seed)["rgba"].copy()
        elif k == "update_textures":
            from bevy_hikari_amd.plugin import encode_texels

            t = self.textures[a["texture"]]
            texels = encode_texels(texture_rectangle(a, op.seed), texture_srgb=base_textures()[a["texture"]]["srgb"])
            t[a["y"]:a["y"] + a["h"], a["x"]:a["x"] + a["w"]] = texels
        elif k == "frame":
            self.frames += 1
        elif k in ("cast_rays", "read_mesh_nodes"):
            pass
        else:
            raise KeyError(k)
        self.raw = [n for n in self.raw if n in self.names() and not self.instances_of(n)]
        self.touch(op.meshes())


# ------------------------------------------------------------------------------------------------------------------------- the generator
def _weights(state, position, length):
    """family weights at `position` of `length`: the calls that end the instance-set family for good (deformations, device poses) are
    rare in the first third and common later, so that a sequence visits the states in front of them first"""
    late = position / max(length - 1, 1)
    unset = any(n in state.instanced() and n not in state.skins for n in SKINNABLE) or any(n in state.instanced() and n not in state.morphs for n in MORPHABLE)
    mesh_set = 3.0 if state.slots == 2 else 8.0 if state.mesh_set_legal() else 0.0   # (one slot: only while the mirrors are fresh, so early and often)
    return dict(mesh_set=mesh_set, instance_set=2.5 if state.instance_ops_legal() else 0.0, poses=1.5, geometry=(1.6 if unset else 0.6) + 3.0 * late, trees=0.4 + 1.2 * late,
                appearance=1.5, observers=2.0)


def _pick(rng, items, recent=(), bias=3.0):
    """one of `items` (a list), those in `recent` `bias` times as likely"""
    items = list(items)
    if not items:
        return None
    w = np.array([bias if it in recent else 1.0 for it in items])
    return items[int(rng.choice(len(items), p=w / w.sum()))]


def _propose(rng, state, family, allowed):
    """an accepted op of `family` in `state`, or None when the family has none"""
    base, seed = state.base, int(rng.integers(1, 1 << 20))
    recent = state.recent
    kinds = [k for k in KINDS if FAMILY[k] == family and k in allowed]
    rng.shuffle(kinds)
    if family == "geometry" and rng.random() < 0.6:   # skins and morph sets first: they deform nothing, and the items that need them come later
        kinds.sort(key=lambda k: k not in ("set_mesh_skin", "set_mesh_morph_targets"))
    for kind in kinds:
        if kind == "add_meshes":
            if not state.mesh_set_legal():
                continue
            free = [n for n in ADDABLE[base] if n not in state.names()]
            if base == "one_slot":
                free = [n for n in free if state.lds_estimate() + 300 * n_triangles(base, n) + 300 < 0.8 * LDS_SCENE_BYTES]
            if not free:
                continue
            count = min(len(free), int(rng.integers(1, 4)))
            chosen = [free[i] for i in sorted(rng.choice(len(free), size=count, replace=False))]
            meshes = [(n, "deferred" if rng.random() < 0.7 else "host") for n in chosen]
            inst = []
            if state.instance_ops_legal() and (base == "two_slot" or rng.random() < 0.5):   # (on one slot the update makes the mirrors stale)
                for n in chosen:
                    if rng.random() < 0.8:
                        inst.append((n, int(rng.integers(0, len(state.materials))), int(rng.integers(1, 1 << 20))))
            op = Op(kind, dict(meshes=meshes, instances=inst), seed)
            if base == "one_slot" and meshes and len(state.instances) + len(inst) > 40:
                continue
            return op
        if kind == "remove_meshes":
            if not state.mesh_set_legal():
                continue
            can_drop = state.instance_ops_legal()
            cands = [m["name"] for m in state.meshes if not m["pinned"] and (can_drop or not state.instances_of(m["name"]))]
            if base == "one_slot":   # (dropping instances makes the mirrors stale: the removal itself would then be refused)
                cands = [n for n in cands if not state.instances_of(n)]
            if not cands:
                continue
            count = min(len(cands), int(rng.integers(1, 4)))
            chosen = []
            for _ in range(count):
                n = _pick(rng, [c for c in cands if c not in chosen], recent)
                chosen.append(n)
            chosen.sort(key=state.mesh_id)
            drop = sorted(i for n in chosen for i in state.instances_of(n))
            return Op(kind, dict(meshes=chosen, drop_instances=drop), seed)
        if kind == "add_instance" and state.instance_ops_legal():
            n = _pick(rng, state.names(), recent)
            return Op(kind, dict(mesh=n, material=int(rng.integers(0, len(state.materials)))), seed)
        if kind == "remove_instance" and state.instance_ops_legal():
            cands = [k for k, i in enumerate(state.instances) if not state.meshes[state.mesh_id(i["mesh"])]["pinned"]]
            if len(cands) and len(state.instances) > 3:
                i = _pick(rng, cands, [k for k in cands if state.instances[k]["mesh"] in recent])
                return Op(kind, dict(instance=i, mesh=state.instances[i]["mesh"]), seed)
        if kind == "set_instance_material" and state.instance_ops_legal():
            i = int(rng.integers(0, len(state.instances)))
            others = [m for m in range(len(state.materials)) if m != state.instances[i]["material"]]
            return Op(kind, dict(instance=i, mesh=state.instances[i]["mesh"], material=others[int(rng.integers(0, len(others)))]), seed)
        if kind in ("refit_instances", "set_instance_transforms"):
            if kind == "refit_instances" and state.device_poses:
                continue
            movable = [k for k, i in enumerate(state.instances) if not state.meshes[state.mesh_id(i["mesh"])]["pinned"]]
            if not movable:
                continue
            if kind == "set_instance_transforms" and rng.random() < 0.5:   # every instance named (ids None): the pinned ones keep their pose
                return Op(kind, dict(ids=None, poses=[(i, int(rng.integers(1, 1 << 20))) for i in movable]), seed)
            count = int(rng.integers(1, min(3, len(movable)) + 1))
            ids = sorted(int(i) for i in rng.choice(movable, size=count, replace=False))
            args = dict(poses=[(i, int(rng.integers(1, 1 << 20))) for i in ids])
            if kind == "set_instance_transforms":
                args["ids"] = ids
            return Op(kind, args, seed)
        if family == "geometry" or kind == "rebuild_mesh_tree":
            # (not the mesh of 40: a deformation takes "exactly the vertices the mesh's triangles span", and three of its vertices no triangle names)
            carried = [n for n in state.instanced() if n in DEFORMABLE or (n in SOUPS and n not in ("s1100", "s40") and kind in ("update_mesh_vertices", "deform_meshes", "deform_meshes_device", "rebuild_mesh_tree"))]
            if kind == "set_mesh_skin":
                cands = [n for n in carried if n in SKINNABLE and n not in state.skins]
                if cands:
                    return Op(kind, dict(mesh=_pick(rng, cands, recent)), seed)
            elif kind == "set_mesh_morph_targets":
                cands = [n for n in carried if n in MORPHABLE and n not in state.morphs]
                if cands:
                    return Op(kind, dict(mesh=_pick(rng, cands, recent)), seed)
            elif kind == "update_mesh_vertices" and carried:
                return Op(kind, dict(mesh=_pick(rng, carried, recent), normals="normals" if rng.random() < 0.6 else "keep"), seed)
            elif kind == "rebuild_mesh_tree":
                cands = [n for n in carried if n in state.history and any(h[0] not in ("set_skin", "set_morph") for h in state.history[n])] or carried
                if cands:
                    return Op(kind, dict(mesh=_pick(rng, cands, recent)), seed)
            elif kind in ("deform_meshes", "deform_meshes_device") and carried:
                count = min(len(carried), int(rng.integers(1, 4)))
                chosen = []
                for _ in range(count):
                    chosen.append(_pick(rng, [c for c in carried if c not in chosen], recent))
                items = []
                for n in chosen:
                    forms = ["vertices"]
                    if n in state.skins:
                        forms.append("skin")
                    if n in state.morphs:
                        forms.append("morph")
                    if n in state.skins and n in state.morphs:
                        forms.append("morph_skin")
                    form = forms[int(rng.integers(0, len(forms)))] if rng.random() < 0.3 else forms[-1]
                    s = int(rng.integers(1, 1 << 20))
                    if form == "vertices":
                        how = ("recompute" if rng.random() < 0.5 else "normals") if kind == "deform_meshes_device" else ("normals" if rng.random() < 0.6 else "keep")
                        items.append(("vertices", n, s, how))
                    else:
                        items.append((form, n, s))
                return Op(kind, dict(items=items), seed)
        if kind == "rebuild_trees":
            return Op(kind, {}, seed)
        if kind == "set_material":
            mid = int(rng.integers(0, len(state.materials)))
            return Op(kind, dict(material=mid, version=state.materials[mid] + 1 + int(rng.integers(0, 3))), seed)
        if kind == "update_texture":
            return Op(kind, dict(texture=int(rng.integers(0, 2))), seed)
        if kind == "update_textures":
            t = int(rng.integers(0, 2))
            th, tw = base_textures()[t]["rgba"].shape[:2]
            w, h = int(rng.integers(1, tw + 1)), int(rng.integers(1, th + 1))
            return Op(kind, dict(texture=t, x=int(rng.integers(0, tw - w + 1)), y=int(rng.integers(0, th - h + 1)), w=w, h=h,
                                 dtype=TEXEL_TYPES[int(rng.integers(0, 3))]), seed)
        if kind in ("frame", "cast_rays", "read_mesh_nodes"):
            return Op(kind, {}, seed)
    return None


def _propose_refusal(rng, state, allowed):
    """an op the table refuses in `state`, marked with its row - or None when the state refuses nothing the generator can name"""
    seed = int(rng.integers(1, 1 << 20))
    rows = []
    if "add_instance" in allowed and (state.deformed or state.device_poses):
        rows.append("instances")
    if "refit_instances" in allowed and state.device_poses:
        rows.append("refit")
    if "remove_meshes" in allowed:
        if any(not m["pinned"] and state.instances_of(m["name"]) for m in state.meshes):
            rows.append("remove_instanced")
        if state.slots == 1 and (state.stale or state.deformed):
            if any(not m["pinned"] and not state.instances_of(m["name"]) for m in state.meshes):
                rows.append("one_slot_remove")
    if "add_meshes" in allowed and state.slots == 1 and (state.stale or state.deformed) and any(n not in state.names() for n in ("s1", "s2", "s3")):
        rows.append("one_slot_add")
    if "deform_meshes" in allowed:
        if any(n in state.instanced() and n not in state.skins for n in SKINNABLE):
            rows.append("skin")
        if any(n in state.instanced() and n not in state.morphs for n in MORPHABLE):
            rows.append("morph")
    if not rows:
        return None
    row = rows[int(rng.integers(0, len(rows)))]
    if row == "instances":
        op = Op("add_instance", dict(mesh=state.names()[0], material=0), seed)
    elif row == "refit":
        op = Op("refit_instances", dict(poses=[(len(state.instances) - 1, seed)]), seed)
    elif row == "remove_instanced":
        n = _pick(rng, [m["name"] for m in state.meshes if not m["pinned"] and state.instances_of(m["name"])], state.recent)
        op = Op("remove_meshes", dict(meshes=[n], drop_instances=[]), seed)
    elif row == "one_slot_remove":
        n = _pick(rng, [m["name"] for m in state.meshes if not m["pinned"] and not state.instances_of(m["name"])], state.recent)
        op = Op("remove_meshes", dict(meshes=[n], drop_instances=[]), seed)
    elif row == "one_slot_add":
        n = [n for n in ("s1", "s2", "s3") if n not in state.names()][0]
        op = Op("add_meshes", dict(meshes=[(n, "deferred")], instances=[]), seed)
    elif row == "skin":
        n = [n for n in SKINNABLE if n in state.instanced() and n not in state.skins][0]
        op = Op("deform_meshes", dict(items=[("skin", n, seed)]), seed)
    else:
        n = [n for n in MORPHABLE if n in state.instanced() and n not in state.morphs][0]
        op = Op("deform_meshes", dict(items=[("morph", n, seed)]), seed)
    op.refuse = state.refusal_row(op)
    assert op.refuse in REFUSALS, (op, row)
    return op


def generate(seed, base, length, kinds=KINDS, refusals=True):
    """The op list of (seed, base): `length` ops, each accepted by the table in the state the ones in front of it leave - or, with
    probability REFUSAL_PROBABILITY, a deliberate refusal marked with its row.  `kinds` narrows the vocabulary and refusals=False leaves the deliberate refusals out (the band test).  The next
    family is drawn by _weights; within it, meshes that recent ops touched are three times as likely as the others."""
    rng = np.random.default_rng([int(seed), BASES.index(base), 20260])
    state, ops = State(base), []
    allowed = set(kinds)
    while len(ops) < length:
        if refusals and rng.random() < REFUSAL_PROBABILITY:
            op = _propose_refusal(rng, state, allowed)
            if op is not None:
                state.apply(op)
                ops.append(op)
                continue
        w = _weights(state, len(ops), length)
        fams = [f for f in FAMILIES if w[f] > 0 and any(FAMILY[k] == f for k in allowed)]
        op = None
        for _ in range(32 if fams else 0):
            p = np.array([w[f] for f in fams])
            op = _propose(rng, state, fams[int(rng.choice(len(fams), p=p / p.sum()))], allowed)
            if op is not None:
                break
        if op is None:
            raise RuntimeError(f"no legal op in state after {ops}")   # (an error in the model: nothing is skipped silently)
        state.apply(op)
        ops.append(op)
    return ops


def replay(ops, base):
    state = State(base)
    for op in ops:
        state.apply(op)
    return state


def accepted_without(ops, base, k):
    """ops without op k if the table still accepts every remaining op in the state it then meets, else None (the reduction step)"""
    rest = ops[:k] + ops[k + 1:]
    try:
        replay(rest, base)
    except (AssertionError, ValueError, IndexError, KeyError):
        return None
    return rest


def end_state(ops, base):
    """What the twin needs, from the ops alone (plain lists and tuples: equal for equal ops, in any process):
      meshes      [(name, how)] in final id order
      instances   [(mesh id, mesh name, material, pose)] in final id order - the last pose of every surviving instance
      materials   [version]; textures: [uint8 arrays]
      history     [(name, [entries])] in id order: per surviving mesh the geometry and tree ops that named it, in order
      flags       the state the live context is in at the end"""
    s = replay(ops, base)
    return dict(base=base,
                meshes=[(m["name"], m["how"]) for m in s.meshes],
                instances=[(s.mesh_id(i["mesh"]), i["mesh"], i["material"], i["pose"]) for i in s.instances],
                materials=list(s.materials), textures=[t.copy() for t in s.textures],
                history=[(m["name"], list(s.history[m["name"]])) for m in s.meshes if m["name"] in s.history],
                flags=dict(stale=s.stale, deformed=s.deformed, device_poses=s.device_poses, skins=sorted(s.skins), morphs=sorted(s.morphs), rebuilt=sorted(s.rebuilt)))


def state_digest(end):
    """a stable text form of an end state (the determinism test compares it across processes)"""
    import hashlib

    h = hashlib.sha256()
    h.update(repr((end["base"], end["meshes"], end["instances"], end["materials"], end["history"], sorted(end["flags"].items()))).encode())
    for t in end["textures"]:
        h.update(t.tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------------------- builders
def add_pool_mesh(builder, base, name, how):
    """how: 'host' (add_mesh), 'deferred' (add_mesh_deferred: the live builder), 'twin' (add_mesh + rebuild_mesh_tree: what the device build of
    a deferred mesh equals)"""
    d = pool(base, name)
    m = builder.add_mesh(d["positions"], d["normals"], d["uvs"], d["indices"], build_tree=how != "deferred")
    if how == "twin":
        builder.rebuild_mesh_tree(m)
    return m


def scene_of(builder, textures):
    scene = builder.finish()
    scene.textures = [dict(rgba=t, srgb=b["srgb"], linear=b["linear"]) for t, b in zip(textures, base_textures())]
    scene.builder = builder
    return scene


def base_builder(base):
    """(finished builder) of a base scene as the live context loads it"""
    from bevy_hikari_amd.plugin import SceneBuilder

    d = base_description(base)
    b = SceneBuilder()
    for k in range(len(d["materials"])):
        b.add_material(material(base, k, 0))
    ids = {name: add_pool_mesh(b, base, name, "host") for name, _ in d["meshes"]}
    for name, mat, p in d["instances"]:
        b.add_instance(ids[name], mat, instance_pose(base, p))
    b.finish()
    return b


def replay_history_on_host(builder, base, mesh_id, entries):
    """a mesh's own geometry and tree history through the host twins: hk_scene_builder_set_mesh_vertices (with the results of hk_morph_vertices and
    the host skinning), recompute_mesh_normals where the device recomputed, rebuild_mesh_tree"""
    for e in entries:
        if e[0] in ("set_skin", "set_morph"):
            continue
        if e[0] == "rebuild":
            builder.rebuild_mesh_tree(mesh_id)
            continue
        p, n = item_result(base, e)
        if e[0] == "vertices" and e[3] == "recompute":
            builder.set_mesh_vertices(mesh_id, p, None)
            builder.recompute_mesh_normals(mesh_id)
        else:
            builder.set_mesh_vertices(mesh_id, p, n)


def end_builder(end, host_geometry):
    """A builder that reaches the end state directly.  host_geometry False: the meshes at rest (the twin context replays the histories on the
    device); True: host_end_builder's."""
    from bevy_hikari_amd.plugin import SceneBuilder

    base = end["base"]
    b = SceneBuilder()
    for k, v in enumerate(end["materials"]):
        b.add_material(material(base, k, v))
    for name, how in end["meshes"]:
        add_pool_mesh(b, base, name, "twin" if how == "deferred" else "host")
    for mesh_id, _, mat, p in end["instances"]:
        b.add_instance(mesh_id, mat, instance_pose(base, p))
    if host_geometry:
        names = [n for n, _ in end["meshes"]]
        b.finish()
        for name, entries in end["history"]:
            replay_history_on_host(b, base, names.index(name), entries)
    b.finish()
    return b


def host_end_builder(ops, base):
    """(finished builder, SceneData with textures) of the end state, built with host calls only: the oracle and the float64 caster read it"""
    end = end_state(ops, base)
    b = end_builder(end, True)
    return b, scene_of(b, end["textures"])
