"""Mesh deformation, host side: the builder's mirror of a device refit (hk_scene_builder_set_mesh_vertices) and the argument checks of
the deformation entry points (hikari_hip.h hk_update_mesh_vertices / hk_set_mesh_skin / hk_skin_mesh).  No GPU needed."""
import ctypes as C

import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder

LEAF = 0x80000000


def leaf_box(prims, shape):
    v = np.array([list(prims[shape].vertices[k].position) for k in range(3)], dtype=np.float32)
    return v.min(axis=0), v.max(axis=0)


def check_union(nodes, prims):
    """every navigator's box = the numpy union of the triangle boxes of the leaves in its subtree (i, exit)"""
    entry = np.array([n.entry_index for n in nodes], dtype=np.int64)
    for i, n in enumerate(nodes):
        if entry[i] >= LEAF:
            assert list(n.min) == [float("inf")] * 3 and list(n.max) == [float("-inf")] * 3, "a leaf keeps the empty box bvh 0.7.1 stores"
            continue
        boxes = [leaf_box(prims, int(entry[j] - LEAF)) for j in range(i + 1, n.exit_index) if entry[j] >= LEAF]
        mn = np.min([b[0] for b in boxes], axis=0)
        mx = np.max([b[1] for b in boxes], axis=0)
        assert np.array_equal(np.array(list(n.min), np.float32), mn) and np.array_equal(np.array(list(n.max), np.float32), mx), f"node {i}"


def mesh_slice(scene, index, arr):
    return arr[index.node_offset:index.node_offset + index.node_count]


def test_set_mesh_vertices_keeps_links_and_refits_every_box():
    b = SceneBuilder()
    p, n, uv, idx = S.cloth_grid(10, 7, size=2.0)
    mesh = b.add_mesh(p, n, uv, idx)
    mat = b.add_material(F.HkMaterial())
    b.add_instance(mesh, mat, np.eye(4, dtype=np.float32).reshape(-1))
    before = b.finish()
    index = b.mesh_index(mesh)
    assert (index.vertex, index.primitive, index.node_offset, index.node_count) == (0, 0, 0, 3 * 140 - 2)
    for frame in (1, 5):
        q, qn = S.waving_cloth(p, frame, amplitude=0.3)
        b.set_mesh_vertices(mesh, q, qn)
        after = b.finish()
        assert [(x.entry_index, x.exit_index) for x in after.asset_nodes] == [(x.entry_index, x.exit_index) for x in before.asset_nodes]
        prims = after.primitives
        for t in range(len(prims)):
            for k in range(3):
                v = prims[t].vertices[k]
                assert list(v.position) == q[v.index].tolist()
        check_union(after.asset_nodes, prims)
        verts = np.array([list(v.position) for v in after.vertices], np.float32)
        assert np.array_equal(verts, q) and np.array_equal(np.array([list(v.normal) for v in after.vertices], np.float32), qn)
        # the instance box follows the new mesh box (identity transform: the box itself)
        lo, hi = q.min(axis=0), q.max(axis=0)
        assert np.allclose(list(after.instances[0].min), lo) and np.allclose(list(after.instances[0].max), hi)
    # normals = NULL keeps them
    b.set_mesh_vertices(mesh, p)
    kept = b.finish()
    assert np.array_equal(np.array([list(v.normal) for v in kept.vertices], np.float32), qn)


def test_builder_mirror_argument_errors():
    api = F.api()
    b = SceneBuilder()
    p, n, uv, idx = S.cloth_grid(2, 2)
    mesh = b.add_mesh(p, n, uv, idx)
    out = F.HkMeshIndex()
    assert api.raw("scene_builder_mesh_index")(b.h, mesh, C.byref(out)) == F.HK_E_INVALID  # not finished since the mesh was added
    b.add_instance(mesh, b.add_material(F.HkMaterial()), np.eye(4, dtype=np.float32).reshape(-1))
    b.finish()
    assert api.raw("scene_builder_mesh_index")(b.h, mesh + 1, C.byref(out)) == F.HK_E_INVALID
    assert api.raw("scene_builder_mesh_index")(b.h, mesh, None) == F.HK_E_INVALID
    fp = p.ctypes.data_as(C.POINTER(F.f32))
    assert api.raw("scene_builder_set_mesh_vertices")(b.h, mesh + 1, fp, None) == F.HK_E_INVALID
    assert api.raw("scene_builder_set_mesh_vertices")(b.h, mesh, None, None) == F.HK_E_INVALID
    assert api.raw("scene_builder_set_mesh_vertices")(None, mesh, fp, None) == F.HK_E_INVALID


def test_device_entry_points_refuse_null_arguments():
    api = F.api()
    mi = F.HkMeshIndex()
    pos = np.zeros((4, 3), np.float32).ctypes.data_as(C.POINTER(F.f32))
    assert api.raw("update_mesh_vertices")(None, C.byref(mi), 4, pos, None) == F.HK_E_INVALID
    assert api.raw("skin_mesh")(None, C.byref(mi), pos, 1) == F.HK_E_INVALID
    assert api.raw("set_mesh_skin")(None, C.byref(mi), 4, pos, pos, None, pos) == F.HK_E_INVALID
    assert api.raw("multi_update_mesh_vertices")(None, C.byref(mi), 4, pos, None) == F.HK_E_INVALID


def test_skin_reference_is_the_identity_for_identity_joints():
    p, n, uv, idx, ji, jw = S.bending_cylinder()
    joints = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (3, 1))
    single = jw.sum(axis=1) == 1.0
    q, qn = S.skin_reference(p, n, ji, jw, joints)
    assert np.array_equal(q[single], p[single]) and np.array_equal(qn[single], n[single])
    assert (jw.sum(axis=1) != 1.0).any() and (jw[:, 1:] == 0).all(axis=1).any(), "the cylinder carries both kinds of weights"


# ---------------------------------------------------------------------------------------------------------------------------------
# Independent references: float64 linear-blend skinning, the distribution an alias table encodes, the -0 < +0 box of a node range
# ---------------------------------------------------------------------------------------------------------------------------------
U32 = np.uint32
EPS32 = 2.0 ** -24
STRESS_VERTICES = 60_003   # 20 001 separate triangles; neither a multiple of 64 nor of 256, 235 blocks of 256 vertices
NODE = np.dtype([("min", "<f4", 3), ("entry", "<u4"), ("max", "<f4", 3), ("exit", "<u4")])


def okey(a):
    """float32 -> uint32 whose unsigned order is the float order with -0 < +0 (the mesh box words of hk_box.hpp, reduced by kernels_deform.hip)"""
    u = np.ascontiguousarray(a, np.float32).view(U32)
    return np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)


def okey_float(k):
    k = np.asarray(k, U32)
    return np.where(k & U32(0x80000000), k & U32(0x7FFFFFFF), ~k).astype(U32).view(np.float32)


def ordered_box(p, axis=0):
    """(min, max) of float32 points under -0 < +0, as float32"""
    k = okey(p)
    return okey_float(k.min(axis=axis)), okey_float(k.max(axis=axis))


def node_array(nodes):
    return np.frombuffer(bytes(nodes), dtype=NODE).copy()


def triangle_boxes(tris):
    """tris float32[t][3][3] -> (lo, hi) float32[t][3] under -0 < +0 (light.wgsl:408-412, the leaf box)"""
    return ordered_box(tris, axis=1)


def expected_node_keys(entry, exit_, tri_lo, tri_hi, filled_leaves):
    """The ordered keys every node of one mesh tree (bvh 0.7.1 flatten_custom, local links) must hold: a navigator i the union of the
    triangle boxes of the leaves in (i, exit); a leaf its own triangle box (filled_leaves: the device) or the empty box (the builder)."""
    n = len(entry)
    leaf = entry >= LEAF
    lo = np.full((n + 1, 3), 0xFFFFFFFF, U32)
    hi = np.zeros((n + 1, 3), U32)
    shape = (entry[leaf] - LEAF).astype(np.int64)
    lo[:n][leaf], hi[:n][leaf] = okey(tri_lo[shape]), okey(tri_hi[shape])
    nav = np.flatnonzero(~leaf)
    out_lo, out_hi = lo[:n].copy(), hi[:n].copy()
    if len(nav):
        seg = np.stack([nav + 1, exit_[nav].astype(np.int64)], 1).reshape(-1)
        assert (exit_[nav] > nav + 1).all() and (exit_[nav] <= n).all()
        out_lo[nav] = np.minimum.reduceat(lo, seg, axis=0)[::2]
        out_hi[nav] = np.maximum.reduceat(hi, seg, axis=0)[::2]
    if not filled_leaves:
        out_lo[leaf], out_hi[leaf] = okey(np.float32(np.inf)), okey(np.float32(-np.inf))
    return out_lo, out_hi


def check_union_fast(nodes, tris, filled_leaves=False, topology=None):
    """check_union for trees of 10^5 triangles: every box of `nodes` (one mesh tree, local links) what expected_node_keys derives from the float32 triangles tris[t][3][3] (index = leaf shape).  topology: the (entry, exit) to read the
    tree by (the builder's, for device nodes whose single-leaf navigators are folded)."""
    a = node_array(nodes)
    entry, exit_ = (a["entry"], a["exit"]) if topology is None else topology
    tri_lo, tri_hi = triangle_boxes(tris)
    lo, hi = expected_node_keys(entry, exit_, tri_lo, tri_hi, filled_leaves)
    # leaves bit for bit; a navigator by value: its union takes std::min / std::max of the children in (left, right) order - the zero of
    # the left child where the two children's bounds are -0 and +0 (scene_builder.cpp refit_nodes, kernels_tree.hip k_lbvh_boxes)
    leaf = entry >= LEAF
    same = lambda got, want: np.where(leaf[:, None], okey(got) == want, got == okey_float(want)).all(1)
    bad = np.flatnonzero(~(same(a["min"], lo) & same(a["max"], hi)))
    assert len(bad) == 0, f"{len(bad)} node boxes differ, first {bad[:8]}"


def stress_joints(n_joints, seed=7):
    """n_joints column-major 4x4 joint matrices: rotations within 0.5 rad of one base rotation, non-uniform scale (0.6-1.6), shear
    (|s| <= 0.3), translations up to 10^3; the upper half of the joints [n // 2, n) mirrored (x negated: det < 0)."""
    rng = np.random.default_rng(seed)
    base, _ = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))
    base *= np.sign(np.linalg.det(base))
    axis = rng.normal(size=(n_joints, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-0.5, 0.5, n_joints)
    K = np.zeros((n_joints, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    K -= K.transpose(0, 2, 1)
    R = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    sh = np.tile(np.eye(3), (n_joints, 1, 1))
    sh[:, 0, 1], sh[:, 0, 2], sh[:, 1, 2] = rng.uniform(-0.3, 0.3, (3, n_joints))
    sc = rng.uniform(0.6, 1.6, (n_joints, 3))
    sc[n_joints // 2:, 0] *= -1.0
    A = base @ R @ sh * sc[:, None, :]
    M = np.zeros((n_joints, 4, 4))
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = A, rng.uniform(-1000.0, 1000.0, (n_joints, 3)), 1.0
    return M.transpose(0, 2, 1).reshape(n_joints, 16).astype(np.float32)


def stress_skin(n_joints, n_vertices=STRESS_VERTICES, seed=11):
    """(bind positions, bind normals, joint indices uint16[n][4], weights float32[n][4]) by vertex kind (v % 4): 0 four non-zero
    weights not summing to one, 1 slot 0 zero and slots 1-3 non-zero, 2 w.w alone, 3 four weights normalised.  A vertex blends joints
    of one half of [0, n_joints) only (stress_joints mirrors the upper half), so the blend stays well conditioned; with 65 536 joints
    every slot names indices >= 256 and >= 0x8000, and joint n_joints - 1 itself."""
    rng = np.random.default_rng(seed)
    n = n_vertices
    p = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    kind = np.arange(n) % 4
    w = rng.uniform(0.1, 1.0, (n, 4))
    w[kind == 1, 0] = 0.0
    w[kind == 2, :3] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    w[kind != 3] *= rng.uniform(0.85, 1.15, ((kind != 3).sum(), 1))
    half = n_joints // 2
    upper = rng.integers(0, 2, n).astype(bool)
    lo_ = np.where(upper, half, 0)[:, None]
    span = np.where(upper, n_joints - half, max(half, 1))[:, None]
    ji = (lo_ + rng.integers(0, 1 << 30, (n, 4)) % span).astype(np.int64)
    for t in range(4):   # joint n_joints - 1 in every slot, by a vertex whose slot t carries weight
        v = np.flatnonzero(upper & (w[:, t] != 0))[t]
        ji[v, t] = n_joints - 1
    assert ji.max() < n_joints
    return p, nrm, ji.astype(np.uint16), w.astype(np.float32)


def lbs64(bind_p, bind_n, ji, jw, joints):
    """float64 linear-blend skinning: M = sum w_t J_t, p' = M (p, 1), n' = inv(M3)^T n; also M3 and the per-component position
    bound 16 eps32 sum_t |w_t| (|J_t| |(p, 1)|)"""
    J = joints.reshape(-1, 4, 4).astype(np.float64).transpose(0, 2, 1)[:, :3, :]   # [joint][row][column]
    w = jw.astype(np.float64)
    Jv = J[ji.astype(np.int64)]                                                      # [v][t][row][column]
    M = np.einsum("vt,vtrc->vrc", w, Jv)
    p1 = np.concatenate([bind_p.astype(np.float64), np.ones((len(bind_p), 1))], 1)
    pos = np.einsum("vrc,vc->vr", M, p1)
    M3 = M[:, :, :3]
    nrm = np.einsum("vji,vj->vi", np.linalg.inv(M3), bind_n.astype(np.float64))
    bound = 16 * EPS32 * np.einsum("vt,vtrc,vc->vr", np.abs(w), np.abs(Jv), np.abs(p1))
    return pos, nrm, M3, bound


def check_against_lbs64(q, qn, bind_p, bind_n, ji, jw, joints):
    """positions within the per-component bound everywhere; normals within 64 eps32 cond(M3) |n64| where cond <= 10^3, and never
    pointing away from the float64 normal"""
    pos, nrm, M3, bound = lbs64(bind_p, bind_n, ji, jw, joints)
    err = np.abs(q.astype(np.float64) - pos)
    assert (err <= bound).all(), f"position off the float64 blend: worst {np.max(err / bound):.3g} x the bound"
    cond = np.linalg.cond(M3)
    ok = cond <= 1e3
    dn = np.linalg.norm(qn.astype(np.float64) - nrm, axis=1)
    lim = 64 * EPS32 * cond * np.linalg.norm(nrm, axis=1)
    assert (dn[ok] <= lim[ok]).all(), f"normal off inv(M3)^T n: worst {np.max(dn[ok] / lim[ok]):.3g} x the bound"
    assert (np.einsum("vi,vi->v", qn.astype(np.float64), nrm) > 0).all()
    return M3, cond


def skin_premises(ji, jw, M3, n_joints):
    """what the stress skin has to exercise (asserted, so that a change of the generator cannot quietly drop a case)"""
    nz = jw != 0
    for t in range(4):
        assert nz[:, t].any() and (ji[nz[:, t], t] >= 256).any(), f"slot {t}"
        if n_joints > 0x8000:
            assert (ji[nz[:, t], t] >= 0x8000).any() and (ji[nz[:, t], t] == n_joints - 1).any(), f"slot {t}"
    assert (nz.all(1) & (np.abs(jw.sum(1) - 1) > 1e-3)).any(), "four weights not summing to one"
    assert (~nz[:, 0] & nz[:, 1:].all(1)).any() and (nz[:, 3] & ~nz[:, :3].any(1)).any()
    det = np.linalg.det(M3)
    assert (det < 0).any() and (det > 0).any(), "mirrored and unmirrored blends"


def test_skin_reference_is_true_linear_blend_skinning():
    """The float32 contract (S.skin_reference, operation for operation the kernel) against float64 LBS on the stress skin: 60 003
    vertices, 65 536 joints - rotations, non-uniform scale, shear, mirrors, translations to 10^3 - and every weight pattern."""
    joints = stress_joints(65536)
    p, n, ji, jw = stress_skin(65536)
    q, qn = S.skin_reference(p, n, ji, jw, joints)
    M3, cond = check_against_lbs64(q, qn, p, n, ji, jw, joints)
    skin_premises(ji, jw, M3, 65536)
    assert (cond <= 1e3).mean() > 0.99
    # the few-joint skins the device test cycles through
    for nj in (3, 300):
        joints = stress_joints(nj)
        p, n, ji, jw = stress_skin(nj, n_vertices=4001)
        q, qn = S.skin_reference(p, n, ji, jw, joints)
        check_against_lbs64(q, qn, p, n, ji, jw, joints)


def alias_distribution(alias):
    """the probability with which light.wgsl:661-664 picks each entry's triangle: slot i uniform (1/n), then the entry's index if
    rand.y < prob, else i itself - P(i) = ((1 - prob_i) + sum over j with index_j = i of prob_j) / n, in float64"""
    prob, index = alias[:, 0].astype(np.float64), alias[:, 1].view(U32).astype(np.int64)
    n = len(alias)
    assert (index < n).all() and (prob >= 0).all() and (prob <= 1).all()
    return ((1.0 - prob) + np.bincount(index, weights=prob, minlength=n)) / n


def world_areas64(p, idx, model):
    """float64 triangle areas after the column-major float32 transform `model`"""
    m = model.reshape(4, 4).T.astype(np.float64)
    w = p.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
    t = w[idx.reshape(-1, 3).astype(np.int64)]
    return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)


def check_alias_distribution(alias, surface_area, areas):
    """an alias table (float32[n][2]: prob, index bits) and surface area against the float64 areas: total variation <= 1e-4, surface
    area within 1e-5 relative, each triangle above 1 % of the mean within 1e-3 relative - but for the one entry the construction leaves
    unpaired.  The reference's loop (mod.rs:353-373, f32) ends when one stack empties, and what is left keeps prob 0: picked with
    1 / n, where its share is 1 - (sum p - n) / n of a slot, and sum p = n sum a / fl(sum a) is off n by n times the rounding of the
    surface area (3.7e-6 x 3 840 = 1.4 % of a slot for a 3 840-triangle sphere).  Its error is bounded by that, plus the pours."""
    assert len(alias) == len(areas)
    n = len(areas)
    P, Q = alias_distribution(alias), areas / areas.sum()
    assert abs(surface_area - areas.sum()) <= 1e-5 * areas.sum()
    assert 0.5 * np.abs(P - Q).sum() <= 1e-4
    untouched = (alias[:, 0] == 0) & (alias[:, 1].view(U32) == np.arange(n))
    left = untouched & (np.abs(Q * n - 1) > 1e-6)
    assert left.sum() <= 1
    assert (np.abs(P - Q)[left] * n <= n * 1e-5 + 1e-3).all()
    big = (areas > 0.01 * areas.mean()) & ~left
    assert (np.abs(P - Q)[big] <= 1e-3 * Q[big]).all(), np.max(np.abs(P - Q)[big] / Q[big])


def emitter_meshes():
    """(name, positions, indices) of emissive meshes for the alias checks: a UV sphere, separate triangles whose areas span four
    decades, one triangle, and a sphere beyond HK_EMITTER_LDS_TRIANGLES (3 264, the device's global-scratch path)"""
    rng = np.random.default_rng(5)
    k = 400
    s = 10.0 ** rng.uniform(0.0, 2.0, k)              # edge lengths over 2 decades: areas over 4
    base = rng.uniform(-50.0, 50.0, (k, 3))
    e1, e2 = rng.normal(size=(k, 3)), rng.normal(size=(k, 3))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 -= np.einsum("ki,ki->k", e2, e1)[:, None] * e1
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    spread = np.stack([base, base + s[:, None] * e1, base + s[:, None] * e2], 1).reshape(-1, 3).astype(np.float32)
    sp, _, _, sidx = S._sphere(8, 12)
    big, _, _, bidx = S._sphere(40, 48)
    one = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.2], [0.3, 0.9, 0.0]], np.float32)
    return [("sphere", sp, sidx), ("spread", spread, np.arange(3 * k, dtype=np.uint32)), ("one", one, np.arange(3, dtype=np.uint32)),
            ("sphere_3840", big, bidx)]


def test_host_alias_tables_encode_the_area_distribution():
    """hk_scene_builder_finish's alias tables (GpuMesh::build_alias_table) pick each triangle with probability area / total, measured
    against float64 world-space areas, for instances under a rotated, non-uniformly scaled transform."""
    b = SceneBuilder()
    glow = b.add_material(S.standard_material((1, 1, 1, 1), (1.0, 0.9, 0.8), 1.0, 0.0, 0.5))
    models, meshes = [], emitter_meshes()
    for i, (name, p, idx) in enumerate(meshes):
        nrm = np.tile(np.array([0, 1, 0], np.float32), (len(p), 1))
        mid = b.add_mesh(p, nrm, np.zeros((len(p), 2), np.float32), idx)
        models.append(S._trs((i, 0.5 * i, -i), (0.3, 0.2 + i, 0.1), (0.5, 1.5, 2.0)))
        b.add_instance(mid, glow, models[-1])
    scene = b.finish()
    alias = np.array([(a.prob, a.index) for a in scene.alias_table], dtype=np.dtype([("p", "<f4"), ("i", "<u4")])).view(np.float32).reshape(-1, 2)
    assert len(scene.emissives) == len(meshes)
    for e, (name, p, idx), model in zip(scene.emissives, meshes, models):
        lo, cnt = e.alias_table
        assert cnt == len(idx) // 3, name
        check_alias_distribution(alias[lo:lo + cnt], e.surface_area, world_areas64(p, idx, model))


def test_set_mesh_vertices_at_scale():
    """The builder's mirror on 130 051 triangles (a 255 x 255 grid and one more triangle: 65 537 vertices): links kept, every
    navigator box the union of its range's triangle boxes (vectorised check_union), -0 / +0 minima and maxima in distant vertices."""
    b = SceneBuilder()
    p, n, uv, idx = big_mesh()
    mesh = b.add_mesh(p, n, uv, idx)
    b.add_instance(mesh, b.add_material(F.HkMaterial()), np.eye(4, dtype=np.float32).reshape(-1))
    before = node_array(b.finish().asset_nodes)
    for frame in (1, 2):
        q = big_mesh_frame(p, frame)
        b.set_mesh_vertices(mesh, q)
        after = b.finish()
        a = node_array(after.asset_nodes)
        assert np.array_equal(a["entry"], before["entry"]) and np.array_equal(a["exit"], before["exit"])
        check_union_fast(after.asset_nodes, q[idx.reshape(-1, 3).astype(np.int64)])
        prims = np.frombuffer(bytes(after.primitives), np.float32).reshape(-1, 3, 4)
        assert np.array_equal(prims[:, :, :3], q[idx.reshape(-1, 3).astype(np.int64)])
        assert np.array_equal(prims[:, :, 3].view(U32), idx.reshape(-1, 3))
        assert np.array_equal(np.array([list(v.position) for v in after.vertices], np.float32), q)


def big_mesh():
    """a 255 x 255-quad grid (65 536 vertices) and one more triangle on a 65 537th vertex: 130 051 triangles"""
    p, n, uv, idx = S.cloth_grid(255, 255, size=2.0)
    p = np.concatenate([p, [[1.1, 0.0, 1.1]]]).astype(np.float32)
    n = np.concatenate([n, [[0.0, 1.0, 0.0]]]).astype(np.float32)
    uv = np.concatenate([uv, [[1.0, 1.0]]]).astype(np.float32)
    idx = np.concatenate([idx, [65535, 65534, 65536]]).astype(np.uint32)
    return p, n, uv, idx


def big_mesh_frame(rest, frame):
    """positions of big_mesh at `frame`: x >= 0 with a +0.0 in block 0 and the minimum -0.0 in block 156; y <= 0 with -0.0 in block 1
    and the maximum +0.0 in block 234; the extremes of z in blocks 3 and 200 (blocks of 256 vertices)"""
    q = rest.astype(np.float64).copy()
    q[:, 0] = np.abs(q[:, 0]) + 0.01 * frame
    q[:, 1] = -np.abs(np.sin(3.0 * q[:, 0] + frame) * np.cos(2.0 * q[:, 2])) - 0.5
    q = q.astype(np.float32)
    q[10, 0], q[40_000, 0] = 0.0, -0.0
    q[300, 1], q[60_000, 1] = -0.0, 0.0
    q[900, 2], q[51_300, 2] = -7.0 - frame, 9.0 + frame
    return q
