"""Shared by test_deform_device.py and test_deform_device_gpu.py: the rule of HK_DEFORM_RECOMPUTE_NORMALS (hikari_hip.h) restated in numpy -
every operation one float32 (or float64) numpy operation, so nothing is contracted - and the small meshes the rule can go wrong on."""
import math

import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.scenes import cloth_grid


def face_vectors(positions, triangles, dtype=np.float32):
    p = np.asarray(positions, dtype=dtype)
    p0, p1, p2 = p[triangles[:, 0]], p[triangles[:, 1]], p[triangles[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(dtype)


def recomputed_normals(positions, triangles, current, dtype=np.float32):
    """s = ((+0 + f[t_1]) + f[t_2]) + ... per vertex over its corners in ascending triangle, then corner order; an all-zero s keeps `current`"""
    f = face_vectors(positions, triangles, dtype)
    s = np.zeros((len(positions), 3), dtype)
    for t in range(len(triangles)):
        for k in range(3):
            v = triangles[t, k]
            s[v] = s[v] + f[t]
    keep = (s == 0).all(axis=1)
    out = s.copy()
    out[keep] = np.asarray(current, dtype=dtype)[keep]
    return out, keep


def mesh_of(scene, index, n_vertices):
    """(positions, normals, triangles) of one mesh of a finished builder's SceneData: the triangles are the vertex indices of its
    HkPrimitive records, in their order - the order the rule is stated in"""
    v = np.frombuffer(bytes(scene.vertices), np.float32).reshape(-1, 8)[index.vertex:index.vertex + n_vertices]
    n_tris = (index.node_count + 2) // 3
    prims = np.frombuffer(bytes(scene.primitives), np.uint32).reshape(-1, 3, 4)[index.primitive:index.primitive + n_tris]
    return v[:, 0:3].copy(), v[:, 4:7].copy(), prims[:, :, 3].astype(np.int64)


def _old_normals(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 3))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def bent_grid():
    """17 x 17 vertices (289: two vertex workgroups), 512 triangles (two triangle workgroups), bent out of its plane"""
    p, _n, uv, idx = cloth_grid(16, 16, size=1.5)
    q = p.astype(np.float64).copy()
    q[:, 1] = 0.25 * np.sin(3.0 * q[:, 0]) * np.cos(2.0 * q[:, 2]) + 0.3 * q[:, 0] ** 2
    return dict(positions=p, normals=_old_normals(len(p), 1), uvs=uv, indices=idx, topology=F.TOPOLOGY_TRIANGLE_LIST, moved=q.astype(np.float32))


def hub_fan():
    """40 triangles round one hub vertex (its normal is a sum of 40 face vectors), the rim not in one plane"""
    rim = [(math.cos(2 * math.pi * k / 40), 0.15 * math.sin(6 * math.pi * k / 40), math.sin(2 * math.pi * k / 40)) for k in range(40)]
    p = np.array([(0.0, 0.0, 0.0)] + rim, np.float32)
    idx = np.array([(0, 1 + (k + 1) % 40, 1 + k) for k in range(40)], np.uint32).reshape(-1)
    q = p.copy()
    q[0] = (0.05, 0.4, -0.03)
    q[1:, 1] *= 1.7
    return dict(positions=p, normals=_old_normals(41, 2), uvs=np.zeros((41, 2), np.float32), indices=idx, topology=F.TOPOLOGY_TRIANGLE_LIST, moved=q)


def zero_area():
    """two triangles and a collinear one (exactly zero face vector: 0, 1, 5 lie on the x axis); vertex 5 is named by that one alone"""
    p = np.array([(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1), (0.5, 0.2, 0.5), (2, 0, 0)], np.float32)
    idx = np.array([0, 2, 1, 1, 2, 3, 0, 1, 5, 2, 4, 3], np.uint32)
    q = p.copy()
    q[4, 1] = 0.6
    q[3, 1] = -0.2
    return dict(positions=p, normals=_old_normals(6, 3), uvs=np.zeros((6, 2), np.float32), indices=idx, topology=F.TOPOLOGY_TRIANGLE_LIST, moved=q)


def unnamed_vertex():
    """vertex 2 lies inside the range and no triangle names it"""
    p = np.array([(0, 0, 0), (1, 0, 0), (7, 7, 7), (0, 0.1, 1), (1, 0, 1)], np.float32)
    idx = np.array([0, 3, 1, 1, 3, 4], np.uint32)
    q = p.copy()
    q[:, 1] += np.array([0.0, 0.3, 0.0, -0.1, 0.2], np.float32)
    return dict(positions=p, normals=_old_normals(5, 4), uvs=np.zeros((5, 2), np.float32), indices=idx, topology=F.TOPOLOGY_TRIANGLE_LIST, moved=q)


def strip():
    """a triangle strip of 9 triangles"""
    p = np.array([(0.2 * (k // 2), 0.05 * math.sin(1.3 * k), 0.3 * (k % 2)) for k in range(11)], np.float32)
    q = p.copy()
    q[:, 1] = np.array([0.12 * math.cos(0.9 * k) for k in range(11)], np.float32)
    return dict(positions=p, normals=_old_normals(11, 5), uvs=np.zeros((11, 2), np.float32), indices=None, topology=F.TOPOLOGY_TRIANGLE_STRIP, moved=q)


def minus_zero():
    """one triangle in the plane x = 1: f.y = e1.z * (+0) - (+0) * e2.z = (-0) - (+0) = -0, and +0 + (-0) stores +0"""
    p = np.array([(1, 0, 0), (1, 1, -1), (1, 0, 1)], np.float32)
    return dict(positions=p, normals=_old_normals(3, 6), uvs=np.zeros((3, 2), np.float32), indices=np.array([0, 1, 2], np.uint32),
                topology=F.TOPOLOGY_TRIANGLE_LIST, moved=p.copy())


CASES = {"bent_grid": bent_grid, "hub_fan": hub_fan, "zero_area": zero_area, "unnamed_vertex": unnamed_vertex, "strip": strip, "minus_zero": minus_zero}
