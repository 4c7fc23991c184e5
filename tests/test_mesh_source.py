"""The host side of hk_add_meshes_device: a mesh DECLARED by its counts (hk_scene_builder_declare_mesh) gets, at the next finish, the
HkMeshIndex a twin that used hk_scene_builder_add_mesh_deferred gets, and once hk_scene_builder_resolve_mesh - the host twin of the
device call, through the same store function - has filled it, the builder holds byte for byte what that twin holds.  Refusals change
nothing."""
import ctypes as C
import re
import subprocess

import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from conftest import ROOT
from test_add_meshes import BUFFERS, record, soup
from test_mesh_rebuild import IDENTITY, flat
from test_scene_load_gpu import assert_builders_equal

LIST, STRIP = F.TOPOLOGY_TRIANGLE_LIST, F.TOPOLOGY_TRIANGLE_STRIP
NAMES = ("hk_scene_builder_declare_mesh", "hk_scene_builder_resolve_mesh", "hk_scene_builder_unresolved_meshes", "hk_add_meshes_device",
         "hk_debug_last_add_sources")


def shapes():
    """(positions, normals, uvs, indices or None, topology) per mesh"""
    rng = np.random.default_rng(5)
    out = []
    p = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    out.append((p, *flat(p), None, LIST))                                    # 1 triangle, non-indexed
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [9, -7, 30], [1, 1, 0]], np.float32)   # vertex 3: unused, outside the triangles' box
    out.append((p, rng.uniform(-1, 1, (5, 3)).astype(np.float32), rng.uniform(0, 1, (5, 2)).astype(np.float32), np.array([0, 1, 2, 2, 1, 4], np.uint32), LIST))
    for n in (3, 4, 5):                                                      # strips: odd triangles flip
        p = rng.uniform(-1, 1, (6, 3)).astype(np.float32)
        out.append((p, *flat(p), rng.permutation(6)[:n].astype(np.uint32), STRIP))
    p, i = soup(257, 9)
    out.append((p, *flat(p), i, LIST))
    p = rng.uniform(-1, 1, (6, 3)).astype(np.float32)                        # -0.0 and subnormals travel as bits
    p[0] = (-0.0, 0.0, -0.0)
    p[1] = np.array([1, 0x807FFFFF, 0x00400000], np.uint32).view(np.float32)
    p[4, 0] = -0.0
    out.append((p, *flat(p), None, LIST))
    p = rng.uniform(-1, 1, (5, 3)).astype(np.float32)                        # a non-indexed strip
    out.append((p, *flat(p), None, STRIP))
    return out


def base():
    b = SceneBuilder()
    b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    p, i = soup(30, 1)
    b.add_instance(b.add_mesh(p, *flat(p), i), 0, IDENTITY)
    return b


def getters(b):
    s = b.scene()
    return {n: bytes(getattr(s, n)) for n in BUFFERS}, b.pending_mesh_trees(), b.unresolved_meshes()


# ---------------------------------------------------------------------------------------------------------------- 1. declared everywhere
def test_the_five_names_and_the_struct_are_declared_everywhere():
    header = open(f"{ROOT}/include/hikari_hip.h").read() + open(f"{ROOT}/include/hikari_hip_debug.h").read()
    rust = open(f"{ROOT}/rust/hikari-hip-sys/src/lib.rs").read()
    exported = subprocess.run(["nm", "-D", "--defined-only", f"{ROOT}/bevy-hikari_amd/libhikari_hip.so"], capture_output=True, text=True, check=True).stdout
    api = F.api()
    assert re.search(r"#define\s+HK_ABI_VERSION\s+8\b", header) and api.abi_version() == 8 and "HK_ABI_VERSION: u32 = 8" in rust
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not in the headers"
        if "_debug_" not in name:   # (the binding is generated from hikari_hip.h: the hooks of hikari_hip_debug.h are not part of it)
            assert re.search(rf"\bpub fn {name}\(", rust), f"{name} is not in the Rust binding"
        assert re.search(rf"\bT {name}\b", exported), f"{name} is not exported"
        assert api.raw(name[3:]).restype is C.c_int
    assert "typedef struct HkMeshSource {" in header and "pub struct HkMeshSource" in rust
    assert C.sizeof(F.HkMeshSource) == 56
    # the offsets of the header's struct, as a C compiler lays it out
    body = re.search(r"typedef struct HkMeshSource \{(.*?)\} HkMeshSource;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    offset, offsets = 0, {}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        size = 8 if "*" in decl else 4
        assert decl.startswith(("uint32_t", "const void*")), decl
        for field in decl.replace("uint32_t", "").replace("const void*", "").split(","):
            offset = (offset + size - 1) // size * size
            offsets[field.strip()] = offset
            offset += size
    assert offset == 56
    assert offsets == {name: getattr(F.HkMeshSource, name).offset for name, _ in F.HkMeshSource._fields_}
    assert len(api.raw("add_meshes_device").argtypes) == 6


# ---------------------------------------------------------------------------------------------------------------- 2. against the twin
def test_declare_finish_resolve_equals_the_deferred_twin():
    d, t = base(), base()
    ids = []
    for p, n, uv, idx, topology in shapes():
        ids.append(d.declare_mesh(len(p), 0 if idx is None else len(idx), topology))
        assert t.add_mesh(p, n, uv, idx, topology, build_tree=False) == ids[-1]
    assert d.unresolved_meshes() == len(ids) and d.pending_mesh_trees() == len(ids)
    d.finish()
    t.finish()
    for m in ids:
        assert record(d.mesh_index(m)) == record(t.mesh_index(m)), f"mesh {m}: the declared mesh's record differs from the deferred twin's"
    for m, (p, n, uv, idx, _) in zip(ids, shapes()):
        d.resolve_mesh(m, p, n, uv, idx)
        d.scene()   # (raises unless the builder is still finished)
    assert d.unresolved_meshes() == 0 and d.pending_mesh_trees() == len(ids)
    assert_builders_equal(d, t, "after resolve_mesh")
    for b in (d, t):   # the mesh box shows in the instance records
        for k, m in enumerate(ids):
            b.add_instance(m, 0, S._trs((0.1 * k, 0.2, -0.1 * k), (0.3, 0.1 * k, 0.0), (1.0, 1.5, 0.5)))
        b.finish()
    assert_builders_equal(d, t, "instances of the resolved meshes")
    for b in (d, t):
        b.build_pending_mesh_trees()
    assert d.pending_mesh_trees() == 0
    assert_builders_equal(d, t, "after build_pending_mesh_trees")


def test_resolve_before_the_finish_and_without_uvs_equals_the_twin():
    d, t = base(), base()
    p, n, uv, idx, topology = shapes()[1]
    m = d.declare_mesh(len(p), len(idx), topology)
    d.resolve_mesh(m, p, n, None, idx)
    assert t.add_mesh(p, n, np.zeros_like(uv), idx, topology, build_tree=False) == m
    d.finish()
    t.finish()
    assert_builders_equal(d, t, "resolved before the finish")


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_change_nothing():
    api = F.api()
    b = base()
    p, n, uv, idx, topology = shapes()[1]
    ordinary = b.add_mesh(p, n, uv, idx, topology)
    declared = b.declare_mesh(len(p), len(idx), topology)
    b.finish()
    before = getters(b)
    out = F.u32(77)
    declare = api.raw("scene_builder_declare_mesh")
    assert declare(b.h, 0, 0, LIST, C.byref(out)) == F.HK_E_INVALID          # no vertices
    assert declare(b.h, 5, 4, LIST, C.byref(out)) == F.HK_E_UNSUPPORTED      # a list of 4 indices
    assert declare(b.h, 4, 0, LIST, C.byref(out)) == F.HK_E_UNSUPPORTED      # ... and the identity list over 4 vertices
    assert declare(b.h, 5, 2, STRIP, C.byref(out)) == F.HK_E_INVALID         # a strip of 2: no triangle
    assert declare(b.h, 5, 3, 7, C.byref(out)) == F.HK_E_UNSUPPORTED         # an unknown topology
    assert declare(None, 3, 0, LIST, C.byref(out)) == F.HK_E_INVALID
    assert out.value == 77
    fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
    ip = lambda a: a.ctypes.data_as(C.POINTER(F.u32))
    resolve = api.raw("scene_builder_resolve_mesh")
    bad = idx.copy()
    bad[-1] = len(p)                                                          # the last corner of the last triangle
    assert resolve(b.h, declared, fp(p), fp(n), fp(uv), ip(bad)) == F.HK_E_INVALID
    assert resolve(b.h, declared, fp(p), fp(n), fp(uv), None) == F.HK_E_INVALID          # declared with indices
    assert resolve(b.h, declared, None, fp(n), fp(uv), ip(idx)) == F.HK_E_INVALID
    assert resolve(b.h, ordinary, fp(p), fp(n), fp(uv), ip(idx)) == F.HK_E_INVALID       # not unresolved
    assert resolve(b.h, 99, fp(p), fp(n), fp(uv), ip(idx)) == F.HK_E_INVALID
    assert api.raw("scene_builder_add_instance")(b.h, declared, 0, (F.f32 * 16)(*IDENTITY.reshape(-1)), None) == F.HK_E_NOT_READY
    assert f"mesh {declared}" in api.last_error()
    assert api.raw("scene_builder_build_pending_mesh_trees")(b.h) == F.HK_E_NOT_READY
    assert f"mesh {declared}" in api.last_error()
    assert api.raw("scene_builder_rebuild_mesh_tree")(b.h, declared) == F.HK_E_NOT_READY
    assert getters(b) == before and before[1:] == (1, 1)
    # the calls that take a context refuse NULL before they look at anything
    assert api.raw("add_meshes_device")(None, b.h, None, 0, F.TREE_SAH, None) == F.HK_E_INVALID
    assert api.raw("debug_last_add_sources")(None, None) == F.HK_E_INVALID
    # ... and the same call with the index mended goes through
    b.resolve_mesh(declared, p, n, uv, idx)
    assert getters(b)[1:] == (1, 0) and getters(b)[0] != before[0]


def test_removing_an_unresolved_mesh_leaves_the_builder_that_never_declared_it():
    d, t = base(), base()
    p, i = soup(12, 3)
    gone = d.declare_mesh(40, 36, LIST)
    for b in (d, t):
        b.add_instance(b.add_mesh(p, *flat(p), i, build_tree=False), 0, IDENTITY)
    d.finish()
    d.remove_mesh(gone)
    assert d.unresolved_meshes() == 0 and d.pending_mesh_trees() == 1
    d.finish()
    t.finish()
    assert_builders_equal(d, t, "after the removal")
