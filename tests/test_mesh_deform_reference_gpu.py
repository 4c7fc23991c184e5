"""Mesh deformation on the device against independent references: what hk_skin_mesh / hk_update_mesh_vertices leave in the vertex and
triangle planes, the mesh box and the mesh tree (hk_debug_read_mesh_geometry, hk_debug_read_mesh_nodes) checked against float64
linear-blend skinning, numpy boxes under the -0 < +0 rule and the float64 area distribution, at the sizes where streaming kernels and
refits go wrong: tens of thousands of vertices over many blocks, 10^5 triangles, 65 536 joints, 1-3 triangles, 70 instances of one
mesh, an emitter beyond the LDS path of k_refit_emitters.  test_mesh_deform_gpu.py holds the frame-by-frame twin comparisons."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from test_mesh_deform import (LEAF, STRESS_VERTICES, U32, big_mesh, big_mesh_frame, check_against_lbs64, check_alias_distribution, check_union_fast,
                              node_array, okey, ordered_box, skin_premises, stress_joints, stress_skin, world_areas64)

pytestmark = pytest.mark.gpu

IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)
SETTINGS = dict(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def mesh_scene(meshes, models=None, emissive=()):
    """A scene of the given meshes [(positions, normals, indices)], one instance each (or one per entry of models[k] for mesh k), with
    the instances whose (mesh, instance) is in `emissive` glowing.  Returns (SceneData with .builder, builder mesh ids, HkMeshIndex
    of each mesh)."""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.6, 0.6, 0.6, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
    ids = [b.add_mesh(p, n, np.zeros((len(p), 2), np.float32), idx) for p, n, idx in meshes]
    for k, mid in enumerate(ids):
        for i, m in enumerate(models[k] if models else [IDENTITY]):
            b.add_instance(mid, glow if (k, i) in emissive else mat, m)
    scene = b.finish()
    scene.builder = b
    return scene, ids, [b.mesh_index(i) for i in ids]


def plugin(flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False):
    if default_traversal:
        with product_default_traversal():
            return hk.HikariPlugin(device=0, flags=flags)
    return hk.HikariPlugin(device=0, flags=flags)


def check_geometry(g, q, qn, idx):
    """device readback == the expected vertices bit for bit; every triangle = the gathered positions with its vertex-index word;
    the mesh box = the numpy min / max under -0 < +0"""
    tri = idx.reshape(-1, 3).astype(np.int64)
    assert np.array_equal(bits(g["positions"]), bits(q)), "positions"
    assert np.array_equal(bits(g["normals"]), bits(qn)), "normals"
    assert np.array_equal(bits(g["triangles"][:, :, :3]), bits(q[tri])), "triangle planes"
    assert np.array_equal(g["triangles"][:, :, 3].view(U32), tri.astype(U32)), "vertex-index words"
    lo, hi = ordered_box(q)
    assert np.array_equal(okey(g["box"][0]), okey(lo)) and np.array_equal(okey(g["box"][1]), okey(hi)), ("mesh box", g["box"], lo, hi)


def stress_mesh():
    p, n, _, jw = stress_skin(3)
    idx = np.random.default_rng(2).permutation(len(p)).astype(np.uint32)   # 20 001 separate triangles, vertices in no order
    return p, n, idx, jw


def test_stress_skin_equals_the_contract_and_float64_lbs():
    """60 003 vertices (235 blocks, the last one partial): the device's skin equals S.skin_reference bit for bit and true LBS within
    the float64 bounds, for 3, 300, 65 536, 3 and 300 joints (the joint matrices' room grows twice and is reused twice)."""
    p, n, idx, jw = stress_mesh()
    assert len(p) == STRESS_VERTICES and len(p) % 64 and len(p) > 256
    scene, _, (index,) = mesh_scene([(p, n, idx)])
    pl = plugin()
    pl.set_scene(scene)
    e = pl.engine
    for nj in (3, 300, 65536, 3, 300):
        ji, joints = stress_skin(nj)[2], stress_joints(nj)
        e.set_mesh_skin(index, p, n, ji, jw)
        e.skin_mesh(index, joints)
        g = e.read_mesh_geometry(index)
        q, qn = S.skin_reference(p, n, ji, jw, joints)
        check_geometry(g, q, qn, idx)
        M3, _ = check_against_lbs64(g["positions"], g["normals"], p, n, ji, jw, joints)
        if nj == 65536:
            skin_premises(ji, jw, M3, nj)


def test_singular_blend_follows_the_contract():
    """All-zero weights (M = 0) and rank-deficient blends (a joint and its mirror half and half; a projection): positions are the
    contract's, normals are non-finite exactly where the contract's are (NaN compared as NaN), finite values bit for bit."""
    rng = np.random.default_rng(9)
    p = rng.uniform(-1, 1, (12, 3)).astype(np.float32)
    n = rng.normal(size=(12, 3)).astype(np.float32)
    idx = np.arange(12, dtype=np.uint32)[::-1].copy()
    ji = np.zeros((12, 4), np.uint16)
    jw = np.zeros((12, 4), np.float32)
    ji[4:8, :2], jw[4:8, :2] = (0, 1), 0.5    # I + mirror: diag(0, 1, 1)
    ji[8:, 2], jw[8:, 2] = 2, 1.0             # a projection onto the xy plane, translated
    joints = np.zeros((3, 4, 4), np.float32)
    joints[0], joints[1], joints[2] = np.eye(4), np.diag([-1.0, 1, 1, 1]), np.diag([1.0, 1, 0, 1])
    joints[2, 3, :3] = (0.5, -2.0, 3.0)       # (column-major: the translation column)
    joints = joints.reshape(3, 16)
    scene, _, (index,) = mesh_scene([(p, n, idx)])
    pl = plugin()
    pl.set_scene(scene)
    e = pl.engine
    e.set_mesh_skin(index, p, n, ji, jw)
    e.skin_mesh(index, joints)
    g = e.read_mesh_geometry(index)
    with np.errstate(divide="ignore", invalid="ignore"):
        q, qn = S.skin_reference(p, n, ji, jw, joints)
    assert (~np.isfinite(qn)).any(axis=1).all(), "every vertex of this skin is singular"
    assert np.isfinite(q).all() and np.array_equal(bits(g["positions"]), bits(q))
    dn = g["normals"]
    assert np.array_equal(np.isnan(dn), np.isnan(qn)), "NaN where the contract has NaN"
    keep = ~np.isnan(qn)
    assert np.array_equal(bits(dn)[keep], bits(qn)[keep]), "non-NaN normals (infinities included) bit for bit"
    tri = idx.reshape(-1, 3).astype(np.int64)
    assert np.array_equal(bits(g["triangles"][:, :, :3]), bits(q[tri]))


def small_mesh(n_vertices, n_tris, seed):
    """random triangles over n_vertices vertices, the first one naming the last vertex (so the mesh spans them all)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_vertices, (n_tris, 3))
    idx[0] = (n_vertices - 1, 0, 1)
    p = rng.uniform(-1, 1, (n_vertices, 3)).astype(np.float32)
    nrm = np.tile(np.array([0, 1, 0], np.float32), (n_vertices, 1))
    return p, nrm, idx.reshape(-1).astype(np.uint32)


def sized_meshes():
    """1, 2 and 3 triangles; 255 / 256 / 257 vertices; 65 537 vertices and 130 051 triangles"""
    out = [small_mesh(3, 1, 1), small_mesh(4, 2, 2), small_mesh(5, 3, 3)] + [small_mesh(nv, 2 * nv, nv) for nv in (255, 256, 257)]
    p, n, _, idx = big_mesh()
    return out + [(p, n, idx)]


def sized_frame(k, rest, frame):
    if len(rest) == 65537:
        return big_mesh_frame(rest, frame)
    rng = np.random.default_rng(100 * frame + k)
    q = rng.uniform(-1.5, 1.5, rest.shape).astype(np.float32)
    if len(q) > 2:   # a -0.0 minimum and a +0.0 maximum in different vertices
        q[:, 0], q[:, 1] = np.abs(q[:, 0]), -np.abs(q[:, 1])
        q[0, 0], q[-1, 0], q[1, 1], q[-2, 1] = 0.0, -0.0, -0.0, 0.0
    return q


@pytest.mark.parametrize("default_traversal", [False, True], ids=["exact", "product_default"])
def test_vertex_updates_at_scale_and_small_edges(default_traversal):
    """hk_update_mesh_vertices with normals, then without (the normals stay), on every mesh of sized_meshes: readback, triangle
    planes and mesh box exact; the mesh nodes of every ordering (1, or 8 threaded) equal the uploaded mirror's; every node of ordering
    0 holds the union of its range's triangle boxes."""
    meshes = sized_meshes()
    scene, ids, indices = mesh_scene(meshes)
    gpu, twin = plugin(default_traversal=default_traversal), plugin(default_traversal=default_traversal)
    gpu.set_scene(scene)
    twin.set_scene(scene)
    b = scene.builder
    topo = [node_array(scene.asset_nodes)[i.node_offset:i.node_offset + i.node_count] for i in indices]
    normals = [m[1] for m in meshes]
    for frame, with_normals in ((1, True), (2, False)):
        data = []
        for k, ((p, n, idx), mid, index) in enumerate(zip(meshes, ids, indices)):
            q = sized_frame(k, p, frame)
            qn = None
            if with_normals:
                qn = np.random.default_rng(k + 50).normal(size=q.shape).astype(np.float32)
                normals[k] = qn
            gpu.engine.update_mesh_vertices(index, q, qn)
            b.set_mesh_vertices(mid, q, qn)
            data.append(q)
        twin.set_scene(b.finish())
        nodes, count, orderings = gpu.engine.read_mesh_nodes()
        tnodes, tcount, torderings = twin.engine.read_mesh_nodes()
        assert (count, orderings) == (tcount, torderings) and orderings == (8 if default_traversal else 1)
        assert bytes(nodes) == bytes(tnodes), f"frame {frame}: mesh nodes differ from the uploaded mirror's"
        dev = node_array(nodes)[:count]   # ordering 0
        for k, ((p, n, idx), index, q) in enumerate(zip(meshes, indices, data)):
            check_geometry(gpu.engine.read_mesh_geometry(index), q, normals[k], idx)
            t = topo[k]
            mine = dev[index.node_offset:index.node_offset + index.node_count]
            check_union_fast(mine.tobytes(), q[idx.reshape(-1, 3).astype(np.int64)], filled_leaves=True, topology=(t["entry"], t["exit"]))


def instance_models(count):
    """identity, uniformly and non-uniformly scaled, rotated, mirrored (one axis or all three), translated instances"""
    out = []
    for i in range(count):
        kind = i % 6
        if kind == 0:
            m = IDENTITY.copy()
        else:
            s = [(2.5, 2.5, 2.5), (0.3, 1.7, 0.9), (1.0, 1.0, 1.0), (-1.0, 1.2, 0.8), (-0.7, -0.7, -0.7)][kind - 1]
            ang = (0.0, 0.0, 0.0) if kind in (1, 2) else (0.3 * i, 0.11 * i, -0.2 * i)
            m = S._trs((0.5 * (i % 9) - 2.0, 0.3 * (i // 9), -0.4 * (i % 5)), ang, s)
        out.append(m)
    return out


def test_many_instances_of_one_deformed_mesh():
    """72 instances of one pulsing sphere (k_mesh_instances over two blocks), 8 of them emitters (emitters first in its list):
    instance boxes equal the mirror's and hold every float64-transformed vertex; emitter records and alias table equal the mirror's."""
    sp, sn, _, sidx = S._sphere(6, 8)
    models = instance_models(72)
    emissive = {(0, i) for i in range(72) if i % 9 == 4}
    scene, (mid,), (index,) = mesh_scene([(sp, sn, sidx)], [models], emissive)
    assert len(scene.emissives) == 8 and len(scene.instances) == 72
    gpu, twin = plugin(), plugin()
    gpu.set_scene(scene)
    twin.set_scene(scene)
    n_t, n_l = len(scene.instance_nodes), len(scene.emissive_nodes)
    for frame in (1, 4):
        q = S.pulsing_sphere(sp, frame) + np.float32(0.01 * frame)
        gpu.engine.update_mesh_vertices(index, q)
        scene.builder.set_mesh_vertices(mid, q)
        twin.set_scene(scene.builder.finish())
        ta, _ = gpu.engine.read_trees(n_t, n_l)
        tb, _ = twin.engine.read_trees(n_t, n_l)
        leaves = lambda t: {n.entry_index - LEAF: (np.array(list(n.min), np.float32), np.array(list(n.max), np.float32)) for n in t if n.entry_index >= LEAF}
        la, lb = leaves(ta), leaves(tb)
        assert sorted(la) == list(range(72)) and sorted(lb) == list(range(72))
        q64 = q.astype(np.float64)
        for i, m in enumerate(models):
            assert np.array_equal(bits(la[i][0]), bits(lb[i][0])) and np.array_equal(bits(la[i][1]), bits(lb[i][1])), f"instance {i} box"
            mm = m.reshape(4, 4).T.astype(np.float64)
            w = q64 @ mm[:3, :3].T + mm[:3, 3]
            lo, hi = la[i][0].astype(np.float64), la[i][1].astype(np.float64)
            tol = 4 * np.spacing(np.maximum(np.abs(la[i][0]), np.abs(la[i][1]))).astype(np.float64)
            assert (w >= lo - tol).all() and (w <= hi + tol).all(), f"instance {i}: a vertex outside its box"
        (ra, aa), (rb, ab) = gpu.engine.read_emitters(), twin.engine.read_emitters()
        assert ra.tobytes() == rb.tobytes() and aa.tobytes() == ab.tobytes(), f"frame {frame}: emitter records / alias table"


def test_deformed_emitter_beyond_the_lds_path():
    """A pulsing emissive sphere of 3 840 triangles (> HK_EMITTER_LDS_TRIANGLES: k_refit_emitters' global scratch): records and the whole
    alias table equal the mirror's, the device's table encodes the float64 area distribution, 3 frames equal the twin's buffers."""
    scene, sun = S.synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    sp, sn, suv, sidx = S._sphere(40, 48)
    mid = b.add_mesh(sp, sn, suv, sidx)
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
    model = S._trs((1.2, 2.0, -0.6), (0.3, 0.5, 0.0), (0.4, 0.6, 0.5))
    b.add_instance(mid, glow, model)
    scene = b.finish()
    index, inst = b.mesh_index(mid), len(scene.instances) - 1
    assert len(sidx) // 3 == 3840 > 3264
    gpu, twin = plugin(), plugin()
    gpu.set_scene(scene)
    twin.set_scene(scene)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for frame in (1, 2, 3):
        q = S.pulsing_sphere(sp, frame + 1)
        gpu.engine.update_mesh_vertices(index, q)
        b.set_mesh_vertices(mid, q)
        twin.set_scene(b.finish())
        (ra, aa), (rb, ab) = gpu.engine.read_emitters(), twin.engine.read_emitters()
        assert ra.tobytes() == rb.tobytes() and aa.tobytes() == ab.tobytes(), f"frame {frame}: emitter records / alias table"
        rec = ra[ra[:, 5].view(U32) == inst]
        assert len(rec) == 1
        off, cnt = rec[0, 6:8].view(U32)
        assert cnt == 3840
        check_alias_distribution(aa[off:off + cnt], float(rec[0, 4]), world_areas64(q, sidx, model))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=frame)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {frame}: {bad}"


def test_bands_skin_the_stress_mesh_like_the_single_context():
    from bevy_hikari_amd.distributed import MultiEngine

    p, n, idx, jw = stress_mesh()
    ji, joints = stress_skin(65536)[2], stress_joints(65536)
    scene, _, (index,) = mesh_scene([(p, n, idx)])
    m, ref = MultiEngine([0, 0], flags=F.CTX_DETERMINISTIC_SCATTER), hk.Engine(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    for t in (m, ref):
        t.upload_noise(); t.upload_scene(scene); t.resize(96, 64, 1.0)
        t.set_mesh_skin(index, p, n, ji, jw)
        t.skin_mesh(index, joints)
    want = ref.read_mesh_geometry(index)
    q, qn = S.skin_reference(p, n, ji, jw, joints)
    check_geometry(want, q, qn, idx)
    bands = m.read_mesh_geometry(index)
    assert len(bands) == 2
    for k, g in enumerate(bands):
        for name in ("positions", "normals", "triangles", "box"):
            assert np.array_equal(bits(g[name]), bits(want[name])), f"band {k}: {name}"
