"""Morph targets (hk_set_mesh_morph_targets, HK_DEFORM_MORPH / HK_DEFORM_MORPH_SKIN, hk_morph_vertices), the half that needs no GPU: the
boundary as every layer states it, and the host twin of the vertex arithmetic against scenes.morph_reference, a numpy float32
restatement - each product and each sum an np.float32 operation rounded on its own.  Every comparison is bit for bit."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.distributed import MultiEngine
from bevy_hikari_amd.plugin import deform_items
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hikari_hip.h")
F32 = np.float32
VERTICES = [1, 3, 64, 65, 259]
TARGETS = [1, 2, 63, 64, 65, 256, 257, 300]


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("positions", "normals")):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5])


def random_set(nv, nt, seed):
    rng = np.random.default_rng(seed)
    bp, bn = rng.standard_normal((nv, 3)).astype(F32), rng.standard_normal((nv, 3)).astype(F32)
    dp, dn = (0.3 * rng.standard_normal((nt, nv, 3))).astype(F32), (0.2 * rng.standard_normal((nt, nv, 3))).astype(F32)
    w = rng.uniform(-0.5, 1.5, nt).astype(F32)
    w[rng.random(nt) < 0.3] = 0.0
    return bp, bn, dp, dn, w


# ---- the boundary
def test_every_layer_declares_the_new_names():
    text = " ".join(re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S).split())
    assert ("int hk_set_mesh_morph_targets(hk_ctx* ctx, const HkMeshIndex* mesh, uint32_t n_vertices, uint32_t n_targets, const float* base_positions, "
            "const float* base_normals, const float* position_deltas, const float* normal_deltas);") in text
    assert ("int hk_multi_set_mesh_morph_targets(hk_multi* m, const HkMeshIndex* mesh, uint32_t n_vertices, uint32_t n_targets, const float* base_positions, "
            "const float* base_normals, const float* position_deltas, const float* normal_deltas);") in text
    assert ("int hk_morph_vertices(uint32_t n_vertices, uint32_t n_targets, const float* base_positions, const float* base_normals, "
            "const float* position_deltas, const float* normal_deltas, const float* weights, float* positions_out, float* normals_out);") in text
    for name, value in (("HK_DEFORM_VERTICES", 0), ("HK_DEFORM_SKIN", 1), ("HK_DEFORM_MORPH", 2), ("HK_DEFORM_MORPH_SKIN", 3), ("HK_MORPH_MAX_TARGETS", 4096)):
        assert re.search(r"#define %s\s+%du\b" % (name, value), text), name
    assert (F.DEFORM_VERTICES, F.DEFORM_SKIN, F.DEFORM_MORPH, F.DEFORM_MORPH_SKIN, F.MORPH_MAX_TARGETS) == (0, 1, 2, 3, 4096)
    fp = C.POINTER(F.f32)
    assert F._PRODUCT_ONLY["set_mesh_morph_targets"] == [C.c_void_p, C.POINTER(F.HkMeshIndex), F.u32, F.u32, fp, fp, fp, fp]
    assert F._PRODUCT_ONLY["multi_set_mesh_morph_targets"] == F._PRODUCT_ONLY["set_mesh_morph_targets"]
    assert F._PRODUCT_ONLY["morph_vertices"] == [F.u32, F.u32] + [fp] * 7
    for name in ("hk_set_mesh_morph_targets", "hk_multi_set_mesh_morph_targets", "hk_morph_vertices"):
        assert name in F.DECLARED_SYMBOLS and hasattr(F.api().dll, name), name
    assert F.DECLARED_SYMBOLS == sorted(F.DECLARED_SYMBOLS)
    assert F.api().abi_version() == 8 and C.sizeof(F.HkMeshDeform) == 40 and C.sizeof(F.HkMeshDeformDevice) == 56   # no struct changes size


def test_generated_rust_crate_and_the_wrappers_carry_the_calls():
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    assert ("pub fn hk_set_mesh_morph_targets(ctx: *mut HkCtx, mesh: *const HkMeshIndex, n_vertices: u32, n_targets: u32, base_positions: *const f32, "
            "base_normals: *const f32, position_deltas: *const f32, normal_deltas: *const f32) -> i32;") in rust
    assert "pub fn hk_multi_set_mesh_morph_targets(m: *mut HkMulti, mesh: *const HkMeshIndex, n_vertices: u32, n_targets: u32," in rust
    assert ("pub fn hk_morph_vertices(n_vertices: u32, n_targets: u32, base_positions: *const f32, base_normals: *const f32, position_deltas: *const f32, "
            "normal_deltas: *const f32, weights: *const f32, positions_out: *mut f32, normals_out: *mut f32) -> i32;") in rust
    for line in ("pub const HK_DEFORM_MORPH: u32 = 2;", "pub const HK_DEFORM_MORPH_SKIN: u32 = 3;", "pub const HK_MORPH_MAX_TARGETS: u32 = 4096;"):
        assert line in rust, line
    text = open(os.path.join(ROOT, "include", "hikari.hpp")).read()
    for call in ("hk_set_mesh_morph_targets(", "hk_multi_set_mesh_morph_targets(", "hk_morph_vertices("):
        assert call in text, call
    names = ["self", "mesh", "base_positions", "base_normals", "position_deltas", "normal_deltas"]
    for cls in (hk.Engine, MultiEngine):
        sig = inspect.signature(cls.set_mesh_morph_targets)
        assert list(sig.parameters) == names and sig.parameters["normal_deltas"].default is None
    assert list(inspect.signature(hk.morph_vertices).parameters) == names[2:] + ["weights"]
    assert list(inspect.signature(S.morph_reference).parameters) == ["base_p", "base_n", "dp", "dn", "weights"]


def test_the_item_tables_carry_the_morph_kinds():
    mesh = F.HkMeshIndex(1, 2, 3, 4)
    w, joints = np.arange(5, dtype=F32), np.tile(np.eye(4, dtype=F32).reshape(-1), (3, 1))
    table, keep = deform_items([("morph", mesh, w), ("morph_skin", mesh, joints, w[:4])])
    assert (table[0].kind, table[0].count, bool(table[0].normals)) == (F.DEFORM_MORPH, 5, False)
    assert [table[0].data[k] for k in range(5)] == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert (table[1].kind, table[1].count) == (F.DEFORM_MORPH_SKIN, 3)
    assert [table[1].normals[k] for k in range(4)] == [0.0, 1.0, 2.0, 3.0] and table[1].data[5] == 1.0
    for bad in (("morph", mesh, w, w), ("morph_skin", mesh, joints)):
        with pytest.raises(ValueError):
            deform_items([bad])


# ---- the host twin
@pytest.mark.parametrize("nv", VERTICES)
def test_host_twin_equals_the_restatement(nv):
    for nt in TARGETS:
        bp, bn, dp, dn, w = random_set(nv, nt, 1000 * nv + nt)
        assert (w == 0).any() or nt < 3
        same(hk.morph_vertices(bp, bn, dp, dn, w), S.morph_reference(bp, bn, dp, dn, w), (nv, nt))
        got = hk.morph_vertices(bp, bn, dp, None, w)
        same(got, (S.morph_reference(bp, bn, dp, None, w)[0], bn), (nv, nt, "no normal deltas"))


def test_scene_targets_and_weights_through_the_twin():
    """the generator the GPU tests use: every mode of the animated weights, with and without normal deltas"""
    p, n, _, _ = S.coil_ribbon(65)
    for nt in (1, 63, 300):
        dp, dn = S.morph_targets(p, n, nt, seed=nt)
        assert dp.shape == dn.shape == (nt, len(p), 3) and dp.dtype == np.float32 and np.abs(dp).max() > 0
        assert S.morph_targets(p, n, nt, normal_deltas=False)[1] is None
        for mode in ("wave", "none", "one", "all", "alternate"):
            w = S.morph_weights(nt, 5, 0.3, mode)
            assert w.dtype == np.float32 and w.shape == (nt,)
            assert int((w != 0).sum()) == {"none": 0, "one": 1, "all": nt, "alternate": (nt + 1) // 2}.get(mode, int((w != 0).sum()))
            same(hk.morph_vertices(p, n, dp, dn, w), S.morph_reference(p, n, dp, dn, w), (nt, mode))
    assert any((S.morph_weights(8, f) == 0).any() for f in range(1, 4)) and (S.morph_weights(8, 2, mode="wave") != 0).any()


def test_zero_weights_give_the_base_exactly():
    bp, bn, dp, dn, _ = random_set(65, 7, 3)
    bp[0, 0], bp[3, 2], bn[1, 1] = -0.0, -0.0, -0.0
    dp[2, 5, 1], dn[4, 6, 0] = np.inf, -np.inf   # an infinite delta under a zero weight leaves no NaN
    for w in (np.zeros(7, F32), np.full(7, -0.0, F32), np.array([0, -0.0, 0, 0, -0.0, 0, 0], F32)):
        got = hk.morph_vertices(bp, bn, dp, dn, w)
        same(got, (bp, bn), "all weights zero")
        same(S.morph_reference(bp, bn, dp, dn, w), (bp, bn), "all weights zero (restatement)")
        assert np.signbit(got[0][0, 0]) and np.signbit(got[0][3, 2]) and np.signbit(got[1][1, 1])
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()


def test_a_negative_zero_weight_is_skipped_and_nan_is_active():
    bp, bn, dp, dn, _ = random_set(5, 4, 4)
    bp[:] = -0.0                      # (-0 + w * d would give +0 for a d of +0 had the target not been skipped)
    dp[1] = 0.0
    dp[1, 2, 0] = np.inf              # -0 * inf = NaN had the product been formed
    w = np.array([0.0, -0.0, 0.0, 0.0], F32)
    got = hk.morph_vertices(bp, bn, dp, dn, w)
    assert np.signbit(got[0]).all() and not np.isnan(got[0]).any()
    w = np.array([0.5, np.nan, 0.0, 2.5], F32)
    got, want = hk.morph_vertices(bp, bn, dp, dn, w), S.morph_reference(bp, bn, dp, dn, w)
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all() and np.isnan(want[0]).all()   # a NaN weight propagates to every vertex
    got, want = hk.morph_vertices(bp, bn, dp, None, w), S.morph_reference(bp, bn, dp, None, w)
    assert np.isnan(got[0]).all() and got[1].tobytes() == bn.tobytes() == want[1].tobytes()


def test_weights_outside_the_unit_interval_are_used_as_given():
    bp, bn, dp, dn, _ = random_set(65, 6, 5)
    w = np.array([-2.5, 1.75, 3.0, -0.125, 1e-30, 100.0], F32)
    got = hk.morph_vertices(bp, bn, dp, dn, w)
    same(got, S.morph_reference(bp, bn, dp, dn, w))
    clamped = hk.morph_vertices(bp, bn, dp, dn, np.clip(w, 0, 1))
    normalised = hk.morph_vertices(bp, bn, dp, dn, w / w.sum())
    assert got[0].tobytes() != clamped[0].tobytes() and got[0].tobytes() != normalised[0].tobytes()


def test_the_sum_runs_in_ascending_target_order():
    """base 1, deltas e, e, 2e with e = 2^-24 (half an ulp of 1) under weights of 1, among skipped targets: ascending
    ((1 + e) + e) + 2e = 1 + 2^-23 (both halves round to even, down), descending ((1 + 2e) + e) + e = 1 + 2^-22 (both round to even, up)."""
    e = F32(2.0 ** -24)
    nt, act = 70, (3, 40, 66)
    bp, bn = np.ones((3, 3), F32), np.ones((3, 3), F32)
    dp = np.full((nt, 3, 3), np.inf, F32)
    for k, d in zip(act, (e, e, F32(2) * e)):
        dp[k] = d
    dn = dp.copy()
    w = np.zeros(nt, F32)
    w[list(act)] = 1.0
    ascending, descending = F32(1.0) + F32(2.0 ** -23), F32(1.0) + F32(2.0 ** -22)
    assert ((F32(1) + e) + e) + F32(2) * e == ascending and ((F32(1) + F32(2) * e) + e) + e == descending and ascending != descending
    got = hk.morph_vertices(bp, bn, dp, dn, w)
    assert (got[0] == ascending).all() and (got[1] == ascending).all()
    same(got, S.morph_reference(bp, bn, dp, dn, w))
    reverse = S.morph_reference(bp, bn, dp[::-1], dn[::-1], w[::-1])
    assert (reverse[0] == descending).all() and got[0].tobytes() != reverse[0].tobytes()


def test_argument_errors_are_refused():
    bp, bn, dp, dn, w = random_set(4, 3, 6)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(F.f32))
    out_p, out_n = np.full_like(bp, 7.0), np.full_like(bn, 7.0)
    raw = F.api().raw("morph_vertices")
    good = [4, 3, fp(bp), fp(bn), fp(dp), fp(dn), fp(w), fp(out_p), fp(out_n)]
    assert raw(*good) == F.HK_OK and out_p.tobytes() == S.morph_reference(bp, bn, dp, dn, w)[0].tobytes()
    out_p[:], out_n[:] = 7.0, 7.0
    for k, value in ((0, 0), (1, 0), (1, F.MORPH_MAX_TARGETS + 1), (2, None), (3, None), (4, None), (6, None), (7, None), (8, None)):
        args = list(good)
        args[k] = value
        assert raw(*args) == F.HK_E_INVALID, k
        assert F.api().last_error()
    assert (out_p == 7.0).all() and (out_n == 7.0).all()   # a refused call writes nothing
    with pytest.raises(ValueError):
        hk.morph_vertices(bp, bn, dp, dn, w[:2])
    with pytest.raises(ValueError):
        hk.morph_vertices(bp, bn[:3], dp, dn, w)
    with pytest.raises(ValueError):
        hk.morph_vertices(bp, bn, dp, dn[:2], w)
