// kernels_scene.hip - instance motion on the device (reference: prepare_instances, instance.rs:286-437).
//
// When an instance moves the reference recomputes, on the CPU, its world AABB and inverse-transpose matrix
// (instance.rs:286-325), the emitter record that follows from them (position, radius, surface area, alias table:
// instance.rs:380-420) and then REBUILDS both acceleration structures - `BVH::build` over all instances and over all
// emitters (instance.rs:365-371,422-428) - before re-uploading every buffer.  Here the per-instance work runs in one
// kernel over the moved instances, reading their new model matrices straight from pinned host memory, and the two
// trees are REFIT in place: same topology (in all eight direction-threaded orderings), every inner box recomputed as the
// union of the leaf boxes below it.  No tree is built and no scene buffer crosses PCIe; the host keeps re-building the
// reference's SAH tree at its leisure (hk_upload_scene_instances, asynchronous) when motion has degraded the refit one.
// This file holds the per-instance side: refit, emitters, the instance boxes, materials and textures.  Building a tree on the device
// (hk_rebuild_scene_trees, the mesh trees) is kernels_tree.hip.
//
// Exactness: everything per instance is the host builder's arithmetic (scene_builder.cpp) operation for operation -
// the double-precision cofactor inverse rounded once, the 8-corner AABB seeded at zero, 0.5 * |cross| triangle areas
// summed in order, the alias-table construction of mod.rs:320-376 - so a refit scene equals what the host path would
// upload for the same tree shape, bit for bit (tests/test_device_refit.py feeds the oracle exactly that).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hk_box.hpp"
#include "hk_device.hpp"
#include "hk_kernels.hpp"

namespace hkd {

namespace {
__device__ __forceinline__ void mat_point(const float* m, const float* p, float* out) {  // glam Mat4::transform_point3
  for (int k = 0; k < 3; ++k) out[k] = m[k] * p[0] + m[4 + k] * p[1] + m[8 + k] * p[2] + m[12 + k];
}
__device__ __forceinline__ void mat_vector(const float* m, const float* p, float* out) {  // glam Mat4::transform_vector3
  for (int k = 0; k < 3; ++k) out[k] = m[k] * p[0] + m[4 + k] * p[1] + m[8 + k] * p[2];
}
// inverse().transpose() in double, rounded once: scene_builder.cpp inverse_transpose, term for term
__device__ bool inverse_transpose(const float* m, float* out) {
  double a[16], inv[16];
  for (int i = 0; i < 16; ++i) a[i] = m[i];
  inv[0] = a[5] * a[10] * a[15] - a[5] * a[11] * a[14] - a[9] * a[6] * a[15] + a[9] * a[7] * a[14] + a[13] * a[6] * a[11] - a[13] * a[7] * a[10];
  inv[4] = -a[4] * a[10] * a[15] + a[4] * a[11] * a[14] + a[8] * a[6] * a[15] - a[8] * a[7] * a[14] - a[12] * a[6] * a[11] + a[12] * a[7] * a[10];
  inv[8] = a[4] * a[9] * a[15] - a[4] * a[11] * a[13] - a[8] * a[5] * a[15] + a[8] * a[7] * a[13] + a[12] * a[5] * a[11] - a[12] * a[7] * a[9];
  inv[12] = -a[4] * a[9] * a[14] + a[4] * a[10] * a[13] + a[8] * a[5] * a[14] - a[8] * a[6] * a[13] - a[12] * a[5] * a[10] + a[12] * a[6] * a[9];
  inv[1] = -a[1] * a[10] * a[15] + a[1] * a[11] * a[14] + a[9] * a[2] * a[15] - a[9] * a[3] * a[14] - a[13] * a[2] * a[11] + a[13] * a[3] * a[10];
  inv[5] = a[0] * a[10] * a[15] - a[0] * a[11] * a[14] - a[8] * a[2] * a[15] + a[8] * a[3] * a[14] + a[12] * a[2] * a[11] - a[12] * a[3] * a[10];
  inv[9] = -a[0] * a[9] * a[15] + a[0] * a[11] * a[13] + a[8] * a[1] * a[15] - a[8] * a[3] * a[13] - a[12] * a[1] * a[11] + a[12] * a[3] * a[9];
  inv[13] = a[0] * a[9] * a[14] - a[0] * a[10] * a[13] - a[8] * a[1] * a[14] + a[8] * a[2] * a[13] + a[12] * a[1] * a[10] - a[12] * a[2] * a[9];
  inv[2] = a[1] * a[6] * a[15] - a[1] * a[7] * a[14] - a[5] * a[2] * a[15] + a[5] * a[3] * a[14] + a[13] * a[2] * a[7] - a[13] * a[3] * a[6];
  inv[6] = -a[0] * a[6] * a[15] + a[0] * a[7] * a[14] + a[4] * a[2] * a[15] - a[4] * a[3] * a[14] - a[12] * a[2] * a[7] + a[12] * a[3] * a[6];
  inv[10] = a[0] * a[5] * a[15] - a[0] * a[7] * a[13] - a[4] * a[1] * a[15] + a[4] * a[3] * a[13] + a[12] * a[1] * a[7] - a[12] * a[3] * a[5];
  inv[14] = -a[0] * a[5] * a[14] + a[0] * a[6] * a[13] + a[4] * a[1] * a[14] - a[4] * a[2] * a[13] - a[12] * a[1] * a[6] + a[12] * a[2] * a[5];
  inv[3] = -a[1] * a[6] * a[11] + a[1] * a[7] * a[10] + a[5] * a[2] * a[11] - a[5] * a[3] * a[10] - a[9] * a[2] * a[7] + a[9] * a[3] * a[6];
  inv[7] = a[0] * a[6] * a[11] - a[0] * a[7] * a[10] - a[4] * a[2] * a[11] + a[4] * a[3] * a[10] + a[8] * a[2] * a[7] - a[8] * a[3] * a[6];
  inv[11] = -a[0] * a[5] * a[11] + a[0] * a[7] * a[9] + a[4] * a[1] * a[11] - a[4] * a[3] * a[9] - a[8] * a[1] * a[7] + a[8] * a[3] * a[5];
  inv[15] = a[0] * a[5] * a[10] - a[0] * a[6] * a[9] - a[4] * a[1] * a[10] + a[4] * a[2] * a[9] + a[8] * a[1] * a[6] - a[8] * a[2] * a[5];
  const double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
  if (det == 0.0) return false;
  const double id = 1.0 / det;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) out[c * 4 + r] = (float)(inv[r * 4 + c] * id);
  return true;
}
// world AABB of an instance (instance.rs:286-305, scene_builder.cpp instance_world_record): the mesh box's 8 corners as vectors, min /
// max seeded at zero, then the centre added.  k_mesh_instances' form of k_refit_instances' arithmetic (which writes it out: keep both in step).
__device__ __forceinline__ void instance_world_box(const float* m, const float* aabb_center, const float* aabb_half, float* mn, float* mx) {
  float center[3];
  mat_point(m, aabb_center, center);
  for (int k = 0; k < 3; ++k) mn[k] = mx[k] = 0.0f;
  for (int corner = 0; corner < 8; ++corner) {
    const float e[3] = {aabb_half[0] * (float)(2 * (corner & 1) - 1), aabb_half[1] * (float)(2 * ((corner >> 1) & 1) - 1),
                        aabb_half[2] * (float)(2 * ((corner >> 2) & 1) - 1)};
    float t[3];
    mat_vector(m, e, t);
    for (int k = 0; k < 3; ++k) {
      mn[k] = hmin(mn[k], t[k]);
      mx[k] = hmax(mx[k], t[k]);
    }
  }
  for (int k = 0; k < 3; ++k) {
    mn[k] = mn[k] + center[k];
    mx[k] = mx[k] + center[k];
  }
}
// a deformed mesh's box (6 order-preserving words, kernels_deform.hip) as bevy's Aabb: Aabb::from_min_max (scene_builder.cpp hk_scene_builder_add_mesh)
__device__ __forceinline__ void mesh_box_of_words(const uint32_t* __restrict__ box, float* aabb_center, float* aabb_half) {
  for (int k = 0; k < 3; ++k) {
    const float mn = box_unword(box[k]), mx = box_unword(box[3 + k]);
    aabb_center[k] = 0.5f * (mx + mn);
    aabb_half[k] = 0.5f * (mx - mn);
  }
}
// the emitter record's position and radius from the instance's world AABB and its material's emissive colour (instance.rs:380-420)
__device__ __forceinline__ float4 emitter_position_radius(const float4 col, const float* mn, const float* mx) {
  const float intensity = 255.0f * col.w * sqrtf(col.x * col.x + col.y * col.y + col.z * col.z);
  float pos[3], d2 = 0.0f;
  for (int k = 0; k < 3; ++k) {
    pos[k] = 0.5f * (mx[k] + mn[k]);
    const float dd = mx[k] - mn[k];
    d2 += dd * dd;
  }
  const float radius = 0.5f * sqrtf(d2) + sqrtf(intensity);
  return make_float4(pos[0], pos[1], pos[2], radius);
}
}  // namespace

// ------------------------------------------------------------------ per moved instance (instance.rs:286-325,380-420)
// One thread per update record.  `failed` receives 1 + instance id of a singular transform (the record is skipped).
__global__ __launch_bounds__(64) void k_refit_instances(RefitScene s, const RefitUpdate* __restrict__ updates, uint32_t n_updates, uint32_t* failed) {
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= n_updates) return;
  const RefitUpdate up = updates[u];
  const uint32_t id = up.instance;
  DInstance& d = s.instances[id];
  if (up.moved == 0u) {  // moved last time, at rest now: its previous model is its model (PreviousMeshUniform)
    d.moved = 0u;
    return;
  }
  float itm[16];
  if (!inverse_transpose(up.model, itm)) {
    if (failed) atomicMax(failed, id + 1u);  // (the host has checked every pose with the same arithmetic: it passes NULL)
    return;
  }
  // previous model = the model this instance was rendered with so far (prepass.wgsl:50,96)
  s.prev_models[4u * id + 0u] = d.m0;
  s.prev_models[4u * id + 1u] = d.m1;
  s.prev_models[4u * id + 2u] = d.m2;
  s.prev_models[4u * id + 3u] = d.m3;
  const float* m = up.model;
  d.im0 = make_float4(itm[0], itm[4], itm[8], itm[12]);  // context.hip build_dynamic_region
  d.im1 = make_float4(itm[1], itm[5], itm[9], itm[13]);
  d.im2 = make_float4(itm[2], itm[6], itm[10], itm[14]);
  d.im3 = make_float4(itm[3], itm[7], itm[11], itm[15]);
  d.m0 = make_float4(m[0], m[1], m[2], m[3]);
  d.m1 = make_float4(m[4], m[5], m[6], m[7]);
  d.m2 = make_float4(m[8], m[9], m[10], m[11]);
  d.m3 = make_float4(m[12], m[13], m[14], m[15]);
  d.n0 = make_float4(itm[0], itm[1], itm[2], 0.0f);
  d.n1 = make_float4(itm[4], itm[5], itm[6], 0.0f);
  d.n2 = make_float4(itm[8], itm[9], itm[10], 0.0f);
  d.moved = 1u;
  // world AABB: the mesh box's 8 corners as vectors, min / max seeded at zero, then the centre added (instance.rs:286-305)
  // (the same arithmetic as instance_world_box / emitter_position_radius, which k_mesh_instances uses: a change here goes there too -
  // written out here because the shared form costs this kernel two VGPRs over its budget, tests/test_kernel_resources.py)
  float center[3];
  mat_point(m, up.aabb_center, center);
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  for (int corner = 0; corner < 8; ++corner) {
    const float e[3] = {up.aabb_half[0] * (float)(2 * (corner & 1) - 1), up.aabb_half[1] * (float)(2 * ((corner >> 1) & 1) - 1),
                        up.aabb_half[2] * (float)(2 * ((corner >> 2) & 1) - 1)};
    float t[3];
    mat_vector(m, e, t);
    for (int k = 0; k < 3; ++k) {
      mn[k] = hmin(mn[k], t[k]);
      mx[k] = hmax(mx[k], t[k]);
    }
  }
  for (int k = 0; k < 3; ++k) {
    mn[k] = mn[k] + center[k];
    mx[k] = mx[k] + center[k];
  }
  s.inst_lo[id] = make_float4(mn[0], mn[1], mn[2], 0.0f);
  s.inst_hi[id] = make_float4(mx[0], mx[1], mx[2], 0.0f);
  const uint32_t e = s.emissive_of_instance[id];
  if (e == HK_U32_MAX) return;
  // the emitter record, instance.rs:380-420
  DEmissive& em = s.emissives[e];
  const float4 col = s.materials[4u * d.material + 1u];
  const float intensity = 255.0f * col.w * sqrtf(col.x * col.x + col.y * col.y + col.z * col.z);
  float pos[3], d2 = 0.0f;
  for (int k = 0; k < 3; ++k) {
    pos[k] = 0.5f * (mx[k] + mn[k]);
    const float dd = mx[k] - mn[k];
    d2 += dd * dd;
  }
  const float radius = 0.5f * sqrtf(d2) + sqrtf(intensity);
  em.position_radius = make_float4(pos[0], pos[1], pos[2], radius);
  // (its area sum and alias table: k_refit_emitters, one WAVE per emitter)
}

// GpuMesh::transformed_primitive_areas (mod.rs:307-318) and build_alias_table (mod.rs:320-376) of every emitter among the update
// records: one WAVE per record (one THREAD per emitter ran all of it until round 3 - O(n) dependent global loads for the
// 2 000-triangle emissive sphere of examples/scene.rs:231-235).  What has to be sequential stays sequential, so every bit is the
// host builder's:
//   1. the n triangle areas: lanes stride over the triangles (independent values, the sequential code's arithmetic each);
//   2. surface_area: ONE lane adds them in index order (f32 addition does not associate);
//   3. the two stacks of the alias construction hold the over- / under-full indices in increasing order: a wave-wide ordered
//      compaction, 64 triangles per step, writes exactly those sequences;
//   4. the pairing loop pops and pushes the stacks one element at a time: one lane - but on stacks that live in LDS whenever the
//      five work arrays fit (n <= 3 264), so its dependent loads cost ~100 cycles instead of a trip to L2 each.
constexpr uint32_t HK_EMITTER_LDS_TRIANGLES = 3264u;  // 5 arrays x 4 B x n <= 65 280 B of dynamic LDS
__global__ __launch_bounds__(64) void k_refit_emitters(RefitScene s, const RefitUpdate* __restrict__ updates, uint32_t n_updates, uint32_t lds_triangles) {
  extern __shared__ __attribute__((aligned(16))) float emitter_lds[];
  const uint32_t u = blockIdx.x, lane = threadIdx.x;
  if (u >= n_updates) return;
  if (updates[u].moved == 0u) return;
  const uint32_t id = updates[u].instance;
  const uint32_t e = s.emissive_of_instance[id];
  if (e == HK_U32_MAX) return;
  float m[16];  // (the records sit in pinned host memory: read once)
  for (int k = 0; k < 16; ++k) m[k] = updates[u].model[k];
  {  // a singular pose leaves the instance record alone (k_refit_instances): then the emitter record stays as well
    float itm[16];
    if (!inverse_transpose(m, itm)) return;
  }
  DEmissive& em = s.emissives[e];
  const uint32_t prim0 = s.instances[id].primitive;
  const uint32_t n = em.alias_count;  // = the mesh's triangle count
  float* work = n <= lds_triangles ? emitter_lds : s.alias_scratch + 5u * (size_t)em.alias_offset;  // (lds_triangles: what the launch reserved)
  float* areas = work;  // [n] areas, then the two stacks (id, prob) x 2
  uint32_t* over_id = reinterpret_cast<uint32_t*>(work + n);
  float* over_p = work + 2u * (size_t)n;
  uint32_t* under_id = reinterpret_cast<uint32_t*>(work + 3u * (size_t)n);
  float* under_p = work + 4u * (size_t)n;
  for (uint32_t i = lane; i < n; i += 64u) {
    const uint32_t prim = prim0 + i;
    const float4 q0 = s.tri_v0[prim], q1 = s.tri_v1[prim], q2 = s.tri_v2[prim];
    const float l0[3] = {q0.x, q0.y, q0.z}, l1[3] = {q1.x, q1.y, q1.z}, l2[3] = {q2.x, q2.y, q2.z};
    float v0[3], v1[3], v2[3];
    mat_point(m, l0, v0);
    mat_point(m, l1, v1);
    mat_point(m, l2, v2);
    const float a[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float b[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    areas[i] = 0.5f * fabsf(sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]));
  }
  __syncthreads();
  float surface_area = 0.0f;
  if (lane == 0u) {
    for (uint32_t i = 0; i < n; ++i) surface_area += areas[i];
    em.surface_area = surface_area;
  }
  surface_area = __shfl(surface_area, 0);
  const float mean_area = surface_area / (float)n;
  uint32_t n_over = 0u, n_under = 0u;  // wave-uniform
  float2* table = s.alias + em.alias_offset;
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t i = base + lane;
    const float p = i < n ? areas[i] / mean_area : 1.0f;
    const unsigned long long mo = __ballot(p > 1.0f), mu = __ballot(p < 1.0f);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (p > 1.0f) {
      const uint32_t at = n_over + (uint32_t)__popcll(mo & below);
      over_id[at] = i;
      over_p[at] = p;
    }
    if (p < 1.0f) {
      const uint32_t at = n_under + (uint32_t)__popcll(mu & below);
      under_id[at] = i;
      under_p[at] = p;
    }
    n_over += (uint32_t)__popcll(mo);
    n_under += (uint32_t)__popcll(mu);
    if (i < n) table[i] = make_float2(0.0f, u2f(i));
  }
  __syncthreads();
  if (lane != 0u) return;
  while (n_under != 0u && n_over != 0u) {
    --n_over;
    const uint32_t oid = over_id[n_over];
    float op = over_p[n_over];
    --n_under;
    const uint32_t uid = under_id[n_under];
    const float upb = under_p[n_under];
    const float delta = 1.0f - upb;
    op -= delta;
    if (op > 1.0f) { over_id[n_over] = oid; over_p[n_over] = op; ++n_over; }
    else if (op < 1.0f) { under_id[n_under] = oid; under_p[n_under] = op; ++n_under; }
    table[uid] = make_float2(delta, u2f(oid));
  }
}

// ------------------------------------------------------------------ refit of a flat skip-link BVH
// One WAVE per node.  A node whose entry carries the leaf flag (a leaf, or a navigator that took over its single leaf's role:
// context.hip fold_leaf_navigators) gets its shape's box; every other node is the navigator of the subtree stored in
// (i, exit): the union of the leaf boxes in that range - min / max are exact, so the order of the union does not matter.
// LIGHT = the light BVH (leaf box = emitter position -/+ radius, light.wgsl:633-636), else the TLAS (leaf box = the
// instance's world AABB, light.wgsl:454-457).  `count` nodes per ordering, `orderings` orderings back to back.
template <bool LIGHT>
__global__ __launch_bounds__(256) void k_refit_flat_bvh(RefitScene s, float4* lo, float4* hi, uint32_t stride /* float4 between lo of consecutive nodes */,
                                                        uint32_t count, uint32_t orderings) {
  const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (wave >= count * orderings) return;
  const uint32_t ord = wave / count, i = wave - ord * count;
  float4* nlo = lo + (size_t)ord * count * stride;
  float4* nhi = hi + (size_t)ord * count * stride;
  auto shape_box = [&](uint32_t shape, f3& mn, f3& mx) {
    if (LIGHT) {
      const float4 pr = s.emissives[shape].position_radius;
      mn = F3(pr.x - pr.w, pr.y - pr.w, pr.z - pr.w);
      mx = F3(pr.x + pr.w, pr.y + pr.w, pr.z + pr.w);
    } else {
      mn = xyz(F4(s.inst_lo[shape]));
      mx = xyz(F4(s.inst_hi[shape]));
    }
  };
  const uint32_t entry = f2u(nlo[(size_t)i * stride].w), exit_ = f2u(nhi[(size_t)i * stride].w);
  f3 mn = F3(INFINITY, INFINITY, INFINITY), mx = F3(-INFINITY, -INFINITY, -INFINITY);
  if (entry >= HK_LEAF) {
    shape_box(entry - HK_LEAF, mn, mx);
  } else {
    for (uint32_t k = i + 1u + lane; k < exit_ && k < count; k += 64u) {
      const uint32_t e = f2u(nlo[(size_t)k * stride].w);
      if (e < HK_LEAF) continue;
      f3 a, b;
      shape_box(e - HK_LEAF, a, b);
      mn = F3(hmin(mn.x, a.x), hmin(mn.y, a.y), hmin(mn.z, a.z));
      mx = F3(hmax(mx.x, b.x), hmax(mx.y, b.y), hmax(mx.z, b.z));
    }
    for (int off = 32; off > 0; off >>= 1) {
      mn = F3(hmin(mn.x, __shfl_xor(mn.x, off)), hmin(mn.y, __shfl_xor(mn.y, off)), hmin(mn.z, __shfl_xor(mn.z, off)));
      mx = F3(hmax(mx.x, __shfl_xor(mx.x, off)), hmax(mx.y, __shfl_xor(mx.y, off)), hmax(mx.z, __shfl_xor(mx.z, off)));
    }
  }
  if (lane == 0u) {
    nlo[(size_t)i * stride] = make_float4(mn.x, mn.y, mn.z, u2f(entry));
    nhi[(size_t)i * stride] = make_float4(mx.x, mx.y, mx.z, u2f(exit_));
  }
}

__global__ __launch_bounds__(256) void k_copy_region_u4(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) dst[i] = src[i];
}
// hk_add_meshes: several copies in one launch, blockIdx.y names the segment (hk_kernels.hpp CopySegments); a tail of whole 4-B words - a
// rank array, the uv plane - goes with the segment's first workgroup
__global__ __launch_bounds__(256) void k_copy_segments(hk::CopySegments t) {
  const hk::CopySegments::Segment s = t.seg[blockIdx.y];
  const size_t n = s.bytes / 16u;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) s.dst[i] = s.src[i];
  const uint32_t tail = (uint32_t)(s.bytes % 16u) / 4u;
  if (blockIdx.x == 0u && threadIdx.x < tail) ((uint32_t*)(s.dst + n))[threadIdx.x] = ((const uint32_t*)(s.src + n))[threadIdx.x];
}
// hk_remove_meshes: the surviving runs of every plane of the mesh level into a new allocation (hk_kernels.hpp CompactArgs).  A workgroup
// takes pieces of HK_COMPACT_PIECE destination bytes, grid-strided; plane and run range of a piece are the same for all its lanes, a
// lane then looks for its run inside that range only - one run however long costs no search, many short ones a short one.  A lane
// moves 16 B where its 16 destination bytes lie in one run and the source is 16-B aligned too (always in the planes of 16 B elements
// and more); in the uv and rank planes, where a removed mesh shifts what follows by 8 or 4 B, and across run boundaries, it moves
// element by element.
__device__ __forceinline__ uint32_t compact_run_of(const hk::CompactRun* __restrict__ runs, uint32_t lo, uint32_t hi, uint32_t elem) {
  while (lo < hi) {  // the last run of [lo, hi] that begins at or in front of elem (runs[lo].dst <= elem)
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (runs[mid].dst <= elem) lo = mid; else hi = mid - 1u;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_compact_planes(hk::CompactArgs a) {
  for (uint64_t piece = blockIdx.x; piece < a.n_pieces; piece += gridDim.x) {
    uint32_t p = 0u;
    for (uint32_t k = 1u; k < a.n_planes; ++k)
      if (a.planes[k].first_piece <= piece) p = k;
    const hk::CompactPlane pl = a.planes[p];
    const hk::CompactRun* __restrict__ runs = a.runs[pl.list];
    const uint32_t n_runs = a.n_runs[pl.list], total = a.total[pl.list], shift = pl.shift;
    const uint64_t bytes = (uint64_t)total << shift;
    const uint64_t b0 = (piece - pl.first_piece) * HK_COMPACT_PIECE;
    const uint64_t b1 = b0 + HK_COMPACT_PIECE < bytes ? b0 + HK_COMPACT_PIECE : bytes;
    if (b0 >= b1 || !n_runs) continue;
    const uint32_t r_lo = compact_run_of(runs, 0u, n_runs - 1u, (uint32_t)(b0 >> shift));
    const uint32_t r_hi = compact_run_of(runs, r_lo, n_runs - 1u, (uint32_t)((b1 - 1u) >> shift));
    for (uint64_t d = b0 + 16u * threadIdx.x; d < b1; d += 16u * 256u) {
      const uint32_t elem = (uint32_t)(d >> shift);
      uint32_t r = compact_run_of(runs, r_lo, r_hi, elem);
      hk::CompactRun run = runs[r];
      if (shift >= 4u) {  // the 16 B are part of one element
        const uint64_t s = ((uint64_t)(run.src + (elem - run.dst)) << shift) + (d & ((1ull << shift) - 1u));
        *(uint4*)(pl.dst + d) = *(const uint4*)(pl.src + s);
        continue;
      }
      const uint32_t per = 16u >> shift, left = total - elem, cnt = left < per ? left : per;
      const uint64_t s = (uint64_t)(run.src + (elem - run.dst)) << shift;
      if (cnt == per && elem + cnt <= run.dst + run.count && (((uintptr_t)(pl.src + s)) & 15u) == 0u) {
        *(uint4*)(pl.dst + d) = *(const uint4*)(pl.src + s);
        continue;
      }
      for (uint32_t j = 0u; j < cnt; ++j) {
        const uint32_t e = elem + j;
        while (e >= run.dst + run.count && r + 1u < n_runs) run = runs[++r];
        const uint64_t from = (uint64_t)(run.src + (e - run.dst)) << shift, to = (uint64_t)e << shift;
        if (shift == 3u) *(uint2*)(pl.dst + to) = *(const uint2*)(pl.src + from);
        else *(uint32_t*)(pl.dst + to) = *(const uint32_t*)(pl.src + from);
      }
    }
  }
}
// ... and the instance-level slot in use into both slots of the new allocation, the three mesh offsets of every DInstance rebased
__global__ __launch_bounds__(256) void k_compact_instances(uint4* __restrict__ dst0, uint4* __restrict__ dst1, const uint4* __restrict__ src, size_t n16, size_t first16,
                                                           uint32_t n_instances, hk::CompactArgs a) {
  static_assert(sizeof(DInstance) == 13 * 16 && offsetof(DInstance, material) == 11 * 16, "the piece that holds material, vertex, primitive, node_offset");
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256u) {
    uint4 v = src[i];
    if (i >= first16 && i - first16 < (size_t)13u * n_instances && (i - first16) % 13u == 11u) {
      v.y = hk::compact_rebase(a.runs[2], a.n_runs[2], v.y);
      v.z = hk::compact_rebase(a.runs[1], a.n_runs[1], v.z);
      v.w = hk::compact_rebase(a.runs[0], a.n_runs[0], v.w);
    }
    dst0[i] = v;
    dst1[i] = v;
  }
}
// hk_add_meshes: reference-layout records (hikari_hip.h HkPrimitive: three 16-B corners; HkVertex: position + u, normal + v) into the
// planes, with the arithmetic of the host layout (scene_layout.hip build_static_region) - pure moves, the normal plane's w is 0
__global__ __launch_bounds__(256) void k_append_geometry(const uint4* __restrict__ prims, uint32_t n_prims, const uint4* __restrict__ verts, uint32_t n_verts,
                                                         float4* __restrict__ v0, float4* __restrict__ v1, float4* __restrict__ v2, float4* __restrict__ vn,
                                                         float2* __restrict__ vuv) {
  auto f4 = [](uint4 u) { return make_float4(u2f(u.x), u2f(u.y), u2f(u.z), u2f(u.w)); };
  const uint32_t step = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_prims; i += step) {
    const uint4 a = prims[3u * (size_t)i], b = prims[3u * (size_t)i + 1u], c = prims[3u * (size_t)i + 2u];
    v0[i] = f4(a);
    v1[i] = f4(b);
    v2[i] = f4(c);
  }
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_verts; i += step) {
    const uint4 a = verts[2u * (size_t)i], b = verts[2u * (size_t)i + 1u];
    vn[i] = make_float4(u2f(b.x), u2f(b.y), u2f(b.z), 0.0f);
    vuv[i] = make_float2(u2f(a.w), u2f(b.w));
  }
}
// world AABB of every instance, from the TLAS leaves of ordering 0 (after a host upload: the refit reads them from here)
__global__ __launch_bounds__(256) void k_gather_instance_boxes(RefitScene s, const float4* __restrict__ tlas, uint32_t count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const float4 lo = tlas[2u * i], hi = tlas[2u * i + 1u];
  const uint32_t entry = f2u(lo.w);
  if (entry < HK_LEAF) return;
  s.inst_lo[entry - HK_LEAF] = make_float4(lo.x, lo.y, lo.z, 0.0f);
  s.inst_hi[entry - HK_LEAF] = make_float4(hi.x, hi.y, hi.z, 0.0f);
}

// ------------------------------------------------------------------ the deformed meshes' new boxes, carried to their instances
// One thread per instance of a deformed mesh, ALL such meshes in one launch (`entries`: pinned, hk_kernels.hpp MeshInstanceEntry - the
// instance, its mesh's box words and the slot of its emitter record): the mesh box (hk_box.hpp box_word, reduced by kernels_deform.hip) as
// bevy's Aabb, the world AABB and emitter record with k_refit_instances' arithmetic (instance_world_box, emitter_position_radius: keep both
// in step) - but the pose, its previous model and its `moved` flag stay as they are (a deformation is no motion of the INSTANCE: the prepass's
// velocity_uv keeps the reference's formula; a mesh that opted in gets per-vertex motion vectors from kernels_motion.hip's pass behind it).  Emitters also get an update record for k_refit_emitters: their triangle areas and alias table follow the new triangles.
__global__ __launch_bounds__(64) void k_mesh_instances(RefitScene s, const MeshInstanceEntry* __restrict__ entries, uint32_t n_entries, RefitUpdate* __restrict__ records) {
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= n_entries) return;
  const MeshInstanceEntry en = entries[u];
  const uint32_t id = en.instance;
  const uint32_t* __restrict__ box = en.box;
  const DInstance& d = s.instances[id];
  const float m[16] = {d.m0.x, d.m0.y, d.m0.z, d.m0.w, d.m1.x, d.m1.y, d.m1.z, d.m1.w, d.m2.x, d.m2.y, d.m2.z, d.m2.w, d.m3.x, d.m3.y, d.m3.z, d.m3.w};
  float ac[3], ah[3];
  mesh_box_of_words(box, ac, ah);
  float mn[3], mx[3];
  instance_world_box(m, ac, ah, mn, mx);
  s.inst_lo[id] = make_float4(mn[0], mn[1], mn[2], 0.0f);
  s.inst_hi[id] = make_float4(mx[0], mx[1], mx[2], 0.0f);
  if (en.record == HK_U32_MAX) return;
  RefitUpdate r;
  r.instance = id;
  r.moved = 1u;
  for (int k = 0; k < 16; ++k) r.model[k] = m[k];
  for (int k = 0; k < 3; ++k) {
    r.aabb_center[k] = ac[k];
    r.aabb_half[k] = ah[k];
  }
  const uint32_t e = s.emissive_of_instance[id];
  if (e == HK_U32_MAX) r.moved = 0u;  // (no emitter after all: k_refit_emitters passes the record by)
  else s.emissives[e].position_radius = emitter_position_radius(s.materials[4u * d.material + 1u], mn, mx);
  records[en.record] = r;
}

// ------------------------------------------------------------------ the instance set changed (hk_change_scene_instances, scene_instances.hip)
// The host has laid the new instance level out in the slot `s` names: counts, offsets, mesh and material words, the emitter list and the
// alias slices are right; poses, boxes and everything derived from them are the host mirrors', which may be stale.  Two kernels put the
// device's own values over them, whatever the number of instances or edits.
// Step 1, poses set from device memory only: a survivor keeps the pose the device holds.  One thread per 16 B: the inverse model, the
// model and the normal matrix - the first 11 float4 of a DInstance - from the record its origin had in the old slot.  The survivor is at
// rest (the host laid `moved` out as 0, so nobody reads a previous model); a new instance keeps the builder's pose.
constexpr uint32_t HK_POSE_PIECES = 11u;
static_assert(offsetof(DInstance, material) == HK_POSE_PIECES * 16u, "the pose of a DInstance is its first 11 float4");
__global__ __launch_bounds__(256) void k_carry_instances(DInstance* __restrict__ now, const DInstance* __restrict__ old, const InstanceDerive* __restrict__ entries,
                                                         uint32_t n_instances) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n_instances * HK_POSE_PIECES) return;
  const uint32_t id = t / HK_POSE_PIECES, piece = t - id * HK_POSE_PIECES;
  const uint32_t origin = entries[id].origin;
  if (origin == HK_U32_MAX) return;
  reinterpret_cast<float4*>(now + id)[piece] = reinterpret_cast<const float4*>(old + origin)[piece];
}
// Step 2, one thread per instance of the new level: its emitter slot into the refit's side array, its world AABB from the pose the slot
// now holds and the mesh's CURRENT box - the device's for a deformed mesh, the builder's otherwise - and for an emitter position and
// radius plus the record k_refit_emitters derives surface area and alias slice from (record e = emitter e).  The arithmetic is
// k_mesh_instances': instance_world_box, emitter_position_radius.
__global__ __launch_bounds__(64) void k_derive_instances(RefitScene s, uint32_t* __restrict__ emissive_of_instance, const InstanceDerive* __restrict__ entries,
                                                         uint32_t n_instances, RefitUpdate* __restrict__ records) {
  const uint32_t id = blockIdx.x * 64u + threadIdx.x;
  if (id >= n_instances) return;
  const InstanceDerive en = entries[id];
  const DInstance& d = s.instances[id];
  const float m[16] = {d.m0.x, d.m0.y, d.m0.z, d.m0.w, d.m1.x, d.m1.y, d.m1.z, d.m1.w, d.m2.x, d.m2.y, d.m2.z, d.m2.w, d.m3.x, d.m3.y, d.m3.z, d.m3.w};
  float ac[3], ah[3];
  if (en.box) mesh_box_of_words(en.box, ac, ah);
  else
    for (int k = 0; k < 3; ++k) {
      ac[k] = en.aabb_center[k];
      ah[k] = en.aabb_half[k];
    }
  float mn[3], mx[3];
  instance_world_box(m, ac, ah, mn, mx);
  s.inst_lo[id] = make_float4(mn[0], mn[1], mn[2], 0.0f);
  s.inst_hi[id] = make_float4(mx[0], mx[1], mx[2], 0.0f);
  emissive_of_instance[id] = en.emitter;
  if (en.emitter == HK_U32_MAX) return;
  RefitUpdate r;
  r.instance = id;
  r.moved = 1u;
  for (int k = 0; k < 16; ++k) r.model[k] = m[k];
  for (int k = 0; k < 3; ++k) {
    r.aabb_center[k] = ac[k];
    r.aabb_half[k] = ah[k];
  }
  s.emissives[en.emitter].position_radius = emitter_position_radius(s.materials[4u * d.material + 1u], mn, mx);
  records[en.emitter] = r;
}

// ------------------------------------------------------------------ poses from device memory (hk_set_instance_transforms_device)
// The host cannot diff poses it never sees: which instance moved is decided here, and k_refit_instances / k_refit_emitters then run
// unchanged over the records written here (launch_refit), as they run over k_mesh_instances' records.
// Phase 1, one thread per instance of the scene: every `moved` flag still set goes (an instance the call does not name is at rest; a
// named one gets its flag back from its record), and the call's status word starts at 0.
__global__ __launch_bounds__(64) void k_pose_begin(RefitScene s, uint32_t n_instances, uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i == 0u && status) *status = 0u;
  if (i >= n_instances) return;
  if (s.instances[i].moved != 0u) s.instances[i].moved = 0u;
}
// Phase 2, one thread per named instance.  named[r] = (instance, index of its pose in the caller's memory), in record order - the host
// puts emitters first (k_refit_emitters runs on the first records only).  The 64 bytes at models + k * stride are compared bit for bit
// with the model the device holds: equal = at rest (a record with moved 0, which every consumer passes by), else the new pose with the
// mesh box from the plane (2 float4 per instance: Aabb centre, half extents).  A pose that is not finite or has no inverse - checked
// with the arithmetic k_refit_instances would use - becomes a record at rest too and reports 1 + its instance id to `status`.
// The pose is read as sixteen floats - the caller owes 4-byte alignment, no more.  The compiler merges them into four 16-byte loads whatever
// the stride: global loads of gfx950 need no more than the element's alignment, so one form serves aligned and odd sources alike.
__global__ __launch_bounds__(64) void k_pose_records(RefitScene s, const uint2* __restrict__ named, uint32_t n_named, const uint8_t* __restrict__ models, uint32_t stride,
                                                     const float4* __restrict__ mesh_boxes, RefitUpdate* __restrict__ records, uint32_t* status) {
  const uint32_t r = blockIdx.x * 64u + threadIdx.x;
  if (r >= n_named) return;
  const uint2 nm = named[r];
  const uint32_t id = nm.x;
  const uint8_t* src = models + (size_t)nm.y * stride;
  const float* f = reinterpret_cast<const float*>(src);
  float4 c[4];
  for (int k = 0; k < 4; ++k) c[k] = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
  const float m[16] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w, c[2].x, c[2].y, c[2].z, c[2].w, c[3].x, c[3].y, c[3].z, c[3].w};
  const DInstance& d = s.instances[id];
  const float4 h[4] = {d.m0, d.m1, d.m2, d.m3};
  uint32_t differs = 0u, finite = 1u;
  for (int k = 0; k < 4; ++k) {
    differs |= (f2u(c[k].x) ^ f2u(h[k].x)) | (f2u(c[k].y) ^ f2u(h[k].y)) | (f2u(c[k].z) ^ f2u(h[k].z)) | (f2u(c[k].w) ^ f2u(h[k].w));
  }
  for (int k = 0; k < 16; ++k)
    if ((f2u(m[k]) & 0x7F800000u) == 0x7F800000u) finite = 0u;
  uint32_t moved = 0u;
  if (differs != 0u) {
    float itm[16];
    if (finite != 0u && inverse_transpose(m, itm)) moved = 1u;
    else if (status) atomicMax(status, id + 1u);
  }
  const float4 bc = mesh_boxes[2u * id], bh = mesh_boxes[2u * id + 1u];
  float4* out = reinterpret_cast<float4*>(records + r);  // (96 bytes per record in a 16-byte aligned array: six 16-byte stores)
  out[0] = make_float4(u2f(id), u2f(moved), m[0], m[1]);
  out[1] = make_float4(m[2], m[3], m[4], m[5]);
  out[2] = make_float4(m[6], m[7], m[8], m[9]);
  out[3] = make_float4(m[10], m[11], m[12], m[13]);
  out[4] = make_float4(m[14], m[15], bc.x, bc.y);
  out[5] = make_float4(bc.z, bh.x, bh.y, bh.z);
}
static_assert(sizeof(RefitUpdate) == 96, "k_pose_records writes a RefitUpdate as six float4");

// ------------------------------------------------------------------ material and texture edits (hk_update_materials, hk_update_texture)
// One thread per changed material: its four float4 from the pinned record into the slot's material array.
__global__ __launch_bounds__(64) void k_write_materials(float4* __restrict__ materials, const MaterialUpdate* __restrict__ updates, uint32_t n_updates) {
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= n_updates) return;
  const uint32_t id = updates[u].material;
  for (int k = 0; k < 4; ++k) materials[4u * id + (uint32_t)k] = updates[u].rows[k];
}
// One thread per emitter whose instance uses a material with a new emissive colour: position and radius again from the instance's
// current box (the refit's side arrays) and the colour k_write_materials has just written - the arithmetic k_mesh_instances uses.
__global__ __launch_bounds__(64) void k_material_emitters(RefitScene s, const uint32_t* __restrict__ emitters, uint32_t n_emitters) {
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= n_emitters) return;
  const uint32_t e = emitters[u];
  const uint32_t id = s.emissives[e].instance;
  const float4 lo = s.inst_lo[id], hi = s.inst_hi[id];
  const float mn[3] = {lo.x, lo.y, lo.z}, mx[3] = {hi.x, hi.y, hi.z};
  s.emissives[e].position_radius = emitter_position_radius(s.materials[4u * s.instances[id].material + 1u], mn, mx);
}
// the texels of one texture from pinned memory (their place in the texel buffer is 4-B aligned, no more), and its descriptor
__global__ __launch_bounds__(256) void k_update_texture(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t n, uint4* info0, uint4* info1, uint4 info) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) dst[i] = src[i];
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    if (info0) *info0 = info;
    if (info1) *info1 = info;
  }
}

// ------------------------------------------------------------------ textures from device memory (hk_update_textures_device)
// The conversion of hikari_hip.h, element by element: host_logic.cpp hk_encode_texels is its twin, operation for operation.
namespace {
__device__ __forceinline__ float texel_clamp(float x) { return x != x ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ uint32_t texel_unorm(float x) { return (uint32_t)__fadd_rn(__fmul_rn(texel_clamp(x), 255.0f), 0.5f); }
// the number of k in 1 .. 255 with v > mid[k] (mid ascends): eight compare steps, no divergence
__device__ __forceinline__ uint32_t texel_srgb(float x, const float* mid) {
  const float v = texel_clamp(x);
  uint32_t k = 0u;
#pragma unroll
  for (uint32_t step = 128u; step; step >>= 1) k += v > mid[k + step] ? step : 0u;
  return k;
}
__device__ __forceinline__ float half_bits(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)h); }  // exact
__device__ __forceinline__ float texel_float(const uint8_t* p, bool half) { return half ? half_bits(*(const unsigned short*)p) : *(const float*)p; }
// one texel of an item: its element(s) at (x, y) of the source, converted and packed r | g << 8 | b << 16 | a << 24
__device__ __forceinline__ uint32_t texel_word(const TextureItem& it, bool encode, bool packed, bool half, const float* mid, uint32_t x, uint32_t y) {
  const uint8_t* p = it.src + (size_t)y * it.stride_y + (size_t)x * it.stride_x;
  if (it.format == HK_TEXELS_U8) {
    if (packed) return *(const uint32_t*)p;
    const uint32_t r = p[0];
    uint32_t g = r, b = r, a = 255u;
    if (it.channels >= 3u) {
      g = p[it.stride_c];
      b = p[2u * it.stride_c];
    }
    if (it.channels == 4u) a = p[3u * it.stride_c];
    return r | (g << 8) | (b << 16) | (a << 24);
  }
  float f0, f1, f2, f3 = 1.0f;
  if (packed && half) {
    const uint2 q = *(const uint2*)p;
    f0 = half_bits(q.x & 0xFFFFu); f1 = half_bits(q.x >> 16); f2 = half_bits(q.y & 0xFFFFu); f3 = half_bits(q.y >> 16);
  } else if (packed) {
    const float4 q = *(const float4*)p;
    f0 = q.x; f1 = q.y; f2 = q.z; f3 = q.w;
  } else {
    f0 = f1 = f2 = texel_float(p, half);
    if (it.channels >= 3u) {
      f1 = texel_float(p + it.stride_c, half);
      f2 = texel_float(p + 2u * it.stride_c, half);
    }
    if (it.channels == 4u) f3 = texel_float(p + 3u * it.stride_c, half);
  }
  const uint32_t r = encode ? texel_srgb(f0, mid) : texel_unorm(f0);
  const uint32_t g = encode ? texel_srgb(f1, mid) : texel_unorm(f1);
  const uint32_t b = encode ? texel_srgb(f2, mid) : texel_unorm(f2);
  const uint32_t a = it.channels == 4u ? texel_unorm(f3) : 255u;
  return r | (g << 8) | (b << 16) | (a << 24);
}
}  // namespace
// One workgroup per span of rows of ONE item's rectangle (hk_kernels.hpp TextureItem, SegmentBlock): lanes run along x, so a wave reads
// whole lines of a CHW plane or contiguous elements of an HWC source, and stores 4 B per lane - contiguous along the row (a texture's
// place in the texel buffer is 4-B aligned and no more, and x0 is arbitrary).  Format, channels and mode are uniform per workgroup.
// (16-B stores of four texels per lane, with single-texel heads and tails per row, were built and measured equal within the noise at
// 1024^2 and 4096^2: profiles/texture_store16_ab.json, profiles/texture_store16_experiment.patch.  The simpler form stayed.)
__global__ __launch_bounds__(256) void k_update_textures(uint32_t* __restrict__ tex_data, const TextureItem* __restrict__ items, const SegmentBlock* __restrict__ blocks,
                                                         const float* __restrict__ thresholds, uint4* info0, uint4* info1) {
  __shared__ float mid[256];
  const SegmentBlock bl = blocks[blockIdx.x];
  const TextureItem& it = items[bl.segment];  // (uniform: read field by field, nothing of it lives in private memory)
  const bool encode = (it.mode & HK_TEXTURE_ITEM_ENCODE) != 0u, packed = (it.mode & HK_TEXTURE_ITEM_PACKED) != 0u;
  if (encode) {
    mid[threadIdx.x] = thresholds[threadIdx.x];
    __syncthreads();
  }
  if (bl.first == 0u && threadIdx.x == 0u) {  // the item's first workgroup: the descriptor, as k_update_texture writes it
    if (info0) info0[it.index] = it.info;
    if (info1) info1[it.index] = it.info;
  }
  const uint32_t rows = min(it.rows, it.height - bl.first);
  const bool half = it.format == HK_TEXELS_F16;
  const uint32_t count = rows * it.width;
  for (uint32_t t = threadIdx.x; t < count; t += 256u) {
    const uint32_t ry = t / it.width, x = t - ry * it.width, y = bl.first + ry;
    tex_data[(size_t)it.dst + (size_t)y * it.pitch + x] = texel_word(it, encode, packed, half, mid, x, y);
  }
}

// hk_add_meshes_device: the reference records (hikari_hip.h HkPrimitive, HkVertex) of many meshes from the caller's arrays.  One workgroup
// per 256 consecutive triangles - the first n_tri_blocks workgroups - or 256 consecutive vertices of ONE source (hk_kernels.hpp
// MeshSourceItem, SegmentBlock), so kind, topology and strides are uniform per workgroup.  Per triangle: 12 B of indices (consecutive
// lanes read consecutive words of a list; a strip's lanes overlap), three 12-B position gathers wherever the indices point, three 16-B
// stores to consecutive 48-B records; per vertex 32 B read at the caller's strides and two 16-B stores.  Pure moves: words, no float
// arithmetic.  An index the mesh does not have is never followed: vertex 0 is read instead and the source is flagged.
__global__ __launch_bounds__(256) void k_assemble_meshes(const MeshSourceItem* __restrict__ items, const SegmentBlock* __restrict__ blocks, uint32_t n_tri_blocks,
                                                         uint32_t* __restrict__ status) {
  const SegmentBlock bl = blocks[blockIdx.x];
  const MeshSourceItem& it = items[bl.segment];  // (uniform: read field by field, nothing of it lives in private memory)
  const uint32_t e = bl.first + threadIdx.x;
  if (blockIdx.x < n_tri_blocks) {
    if (e >= it.n_tris) return;
    size_t a = 3u * (size_t)e, b = a + 1u, c = a + 2u;
    if (it.strip) {
      a = (size_t)e + (e & 1u);
      b = (size_t)e + 1u - (e & 1u);
      c = (size_t)e + 2u;
    }
    uint32_t id[3] = {(uint32_t)a, (uint32_t)b, (uint32_t)c};
    if (it.indices) {
      id[0] = it.indices[a];
      id[1] = it.indices[b];
      id[2] = it.indices[c];
    }
    if (id[0] >= it.n_vertices || id[1] >= it.n_vertices || id[2] >= it.n_vertices) atomicMin(status, bl.segment);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t v = id[k] < it.n_vertices ? id[k] : 0u;
      const uint32_t* p = (const uint32_t*)(it.positions + (size_t)v * it.stride_p);
      it.prims[3u * (size_t)e + k] = make_uint4(p[0], p[1], p[2], id[k]);
    }
    return;
  }
  if (e >= it.n_vertices) return;
  const uint32_t* p = (const uint32_t*)(it.positions + (size_t)e * it.stride_p);
  const uint32_t* n = (const uint32_t*)(it.normals + (size_t)e * it.stride_n);
  uint32_t u = 0u, v = 0u;  // (+0.0f)
  if (it.uvs) {
    const uint32_t* t = (const uint32_t*)(it.uvs + (size_t)e * it.stride_uv);
    u = t[0];
    v = t[1];
  }
  it.verts[2u * (size_t)e] = make_uint4(p[0], p[1], p[2], u);
  it.verts[2u * (size_t)e + 1u] = make_uint4(n[0], n[1], n[2], v);
}

}  // namespace hkd

namespace hk {
using namespace hkd;

// the tail of every update: the instance tree refit in all its orderings (interleaved lo / hi pairs), then the light tree (two planes)
static void launch_refit_trees(hipStream_t st, const RefitScene& s, float4* tlas, uint32_t tlas_count, uint32_t orderings, float4* light_lo, float4* light_hi,
                               uint32_t light_count) {
  if (tlas_count) {
    const uint32_t waves = tlas_count * orderings;
    hipLaunchKernelGGL((k_refit_flat_bvh<false>), dim3((waves + 3u) / 4u), dim3(256), 0, st, s, tlas, tlas + 1, 2u, tlas_count, orderings);
  }
  if (light_count) hipLaunchKernelGGL((k_refit_flat_bvh<true>), dim3((light_count + 3u) / 4u), dim3(256), 0, st, s, light_lo, light_hi, 1u, light_count, 1u);
}

void launch_material_update(hipStream_t st, const RefitScene& s, float4* materials, const MaterialUpdate* updates, uint32_t n_updates, const uint32_t* emitters,
                            uint32_t n_emitters, float4* light_lo, float4* light_hi, uint32_t light_count) {
  if (n_updates) hipLaunchKernelGGL(k_write_materials, dim3((n_updates + 63u) / 64u), dim3(64), 0, st, materials, updates, n_updates);
  if (!n_emitters) return;
  hipLaunchKernelGGL(k_material_emitters, dim3((n_emitters + 63u) / 64u), dim3(64), 0, st, s, emitters, n_emitters);
  launch_refit_trees(st, s, nullptr, 0u, 0u, light_lo, light_hi, light_count);
}
void launch_texture_update(hipStream_t st, uint32_t* dst, const uint32_t* src, size_t n, uint4* info0, uint4* info1, uint4 info) {
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096));
  hipLaunchKernelGGL(k_update_texture, dim3(blocks), dim3(256), 0, st, dst, src, n, info0, info1, info);
}
uint32_t launch_textures_update(hipStream_t st, uint32_t* tex_data, const TextureItem* items, const SegmentBlock* blocks, uint32_t n_blocks, const float* thresholds,
                                uint4* info0, uint4* info1, hipEvent_t sources_read) {
  if (!n_blocks) return 0u;
  hipLaunchKernelGGL(k_update_textures, dim3(n_blocks), dim3(256), 0, st, tex_data, items, blocks, thresholds, info0, info1);
  if (sources_read) (void)hipEventRecord(sources_read, st);
  return 1u;
}

void launch_copy_region(hipStream_t st, void* dst, const void* src, size_t bytes) {
  const size_t n = bytes / 16;
  if (!n) return;
  hipLaunchKernelGGL(k_copy_region_u4, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, (uint4*)dst, (const uint4*)src, n);
}
void launch_copy_segments(hipStream_t st, const CopySegments& segments) {
  if (!segments.count || segments.overflow) return;
  size_t longest = 0;
  for (uint32_t k = 0; k < segments.count; ++k) longest = std::max(longest, segments.seg[k].bytes / 16);
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((longest + 255) / 256, 2048));
  hipLaunchKernelGGL(k_copy_segments, dim3(blocks, segments.count), dim3(256), 0, st, segments);
}
void launch_compact_planes(hipStream_t st, const CompactArgs& a, int compute_units) {
  if (!a.n_pieces) return;
  // (a capped grid, the rest strided: a few workgroups per compute unit keep the memory system busy, more only add launch overhead)
  const uint64_t cap = (uint64_t)std::max(compute_units, 64) * 8u;
  hipLaunchKernelGGL(k_compact_planes, dim3((unsigned)std::min<uint64_t>(a.n_pieces, cap)), dim3(256), 0, st, a);
}
void launch_compact_instances(hipStream_t st, uint4* dst0, uint4* dst1, const uint4* src, size_t n16, size_t first16, uint32_t n_instances, const CompactArgs& a) {
  if (!n16) return;
  hipLaunchKernelGGL(k_compact_instances, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 2048)), dim3(256), 0, st, dst0, dst1, src, n16, first16, n_instances, a);
}
void launch_append_geometry(hipStream_t st, const uint4* prims, uint32_t n_prims, const uint4* verts, uint32_t n_verts, float4* v0, float4* v1, float4* v2, float4* vn,
                            float2* vuv) {
  const uint32_t n = std::max(n_prims, n_verts);
  if (!n) return;
  hipLaunchKernelGGL(k_append_geometry, dim3(std::min((n + 255u) / 256u, 4096u)), dim3(256), 0, st, prims, n_prims, verts, n_verts, v0, v1, v2, vn, vuv);
}
uint32_t launch_assemble_meshes(hipStream_t st, const MeshSourceItem* items, const SegmentBlock* blocks, uint32_t n_tri_blocks, uint32_t n_blocks, uint32_t* status,
                                hipEvent_t sources_read) {
  if (!n_blocks) return 0u;
  hipLaunchKernelGGL(k_assemble_meshes, dim3(n_blocks), dim3(256), 0, st, items, blocks, n_tri_blocks, status);
  if (sources_read) (void)hipEventRecord(sources_read, st);
  return 1u;
}
void launch_gather_instance_boxes(hipStream_t st, const RefitScene& s, const float4* tlas, uint32_t tlas_count) {
  if (!tlas_count) return;
  hipLaunchKernelGGL(k_gather_instance_boxes, dim3((tlas_count + 255u) / 256u), dim3(256), 0, st, s, tlas, tlas_count);
}
void launch_refit(hipStream_t st, const RefitScene& s, const RefitUpdate* updates, uint32_t n_updates, uint32_t n_emitter_updates, uint32_t emitter_triangles,
                  uint32_t* failed, float4* tlas, uint32_t tlas_count,
                  uint32_t orderings, float4* light_lo, float4* light_hi, uint32_t light_count) {
  if (n_updates) {
    hipLaunchKernelGGL(k_refit_instances, dim3((n_updates + 63u) / 64u), dim3(64), 0, st, s, updates, n_updates, failed);
    // the host puts the records of moved EMITTERS first: one workgroup (= one wave) per such record only, with the LDS its largest
    // mesh needs (a 64 KB reservation on thousands of workgroups that exit at once capped everybody's occupancy)
    if (n_emitter_updates) {
      const uint32_t lds_triangles = std::min(emitter_triangles, HK_EMITTER_LDS_TRIANGLES);
      hipLaunchKernelGGL(k_refit_emitters, dim3(n_emitter_updates), dim3(64), lds_triangles * 5u * 4u, st, s, updates, n_emitter_updates, lds_triangles);
    }
  }
  launch_refit_trees(st, s, tlas, tlas_count, orderings, light_lo, light_hi, light_count);
}

uint32_t launch_pose_records(hipStream_t st, const RefitScene& s, uint32_t n_instances, const uint2* named, uint32_t n_named, const void* models, uint32_t stride,
                             const float4* mesh_boxes, RefitUpdate* records, uint32_t* status, hipEvent_t sources_read) {
  if (!n_instances) return 0u;
  hipLaunchKernelGGL(k_pose_begin, dim3((n_instances + 63u) / 64u), dim3(64), 0, st, s, n_instances, status);
  if (!n_named) return 1u;
  hipLaunchKernelGGL(k_pose_records, dim3((n_named + 63u) / 64u), dim3(64), 0, st, s, named, n_named, (const uint8_t*)models, stride, mesh_boxes, records, status);
  if (sources_read) (void)hipEventRecord(sources_read, st);  // (the last launch that reads the caller's memory)
  return 2u;
}

uint32_t launch_instance_change(hipStream_t st, const RefitScene& s, uint32_t* emissive_of_instance, const DInstance* old_instances, const InstanceDerive* entries,
                                uint32_t n_instances, RefitUpdate* records, uint32_t n_emitters, uint32_t emitter_triangles, float4* tlas, uint32_t tlas_count, uint32_t orderings,
                                float4* light_lo, float4* light_hi, uint32_t light_count) {
  if (!n_instances) return 0u;
  uint32_t launches = 1u;
  if (old_instances) {
    hipLaunchKernelGGL(k_carry_instances, dim3((n_instances * HK_POSE_PIECES + 255u) / 256u), dim3(256), 0, st, s.instances, old_instances, entries, n_instances);
    ++launches;
  }
  hipLaunchKernelGGL(k_derive_instances, dim3((n_instances + 63u) / 64u), dim3(64), 0, st, s, emissive_of_instance, entries, n_instances, records);
  if (n_emitters) {  // one workgroup (= one wave) per emitter record, with the LDS the largest of their meshes needs
    const uint32_t lds_triangles = std::min(emitter_triangles, HK_EMITTER_LDS_TRIANGLES);
    hipLaunchKernelGGL(k_refit_emitters, dim3(n_emitters), dim3(64), lds_triangles * 5u * 4u, st, s, (const RefitUpdate*)records, n_emitters, lds_triangles);
    ++launches;
  }
  launch_refit_trees(st, s, tlas, tlas_count, orderings, light_lo, light_hi, light_count);
  return launches + (tlas_count ? 1u : 0u) + (light_count ? 1u : 0u);
}

uint32_t launch_mesh_propagate(hipStream_t st, const RefitScene& s, const MeshInstanceEntry* entries, uint32_t n_entries, RefitUpdate* records, uint32_t n_emitters,
                               uint32_t emitter_triangles, float4* tlas, uint32_t tlas_count, uint32_t orderings, float4* light_lo, float4* light_hi, uint32_t light_count) {
  uint32_t launches = 0u;
  if (n_entries) {
    hipLaunchKernelGGL(k_mesh_instances, dim3((n_entries + 63u) / 64u), dim3(64), 0, st, s, entries, n_entries, records);
    ++launches;
  }
  if (n_emitters) {  // one workgroup (= one wave) per emitter record, with the LDS the largest of their meshes needs
    const uint32_t lds_triangles = std::min(emitter_triangles, HK_EMITTER_LDS_TRIANGLES);
    hipLaunchKernelGGL(k_refit_emitters, dim3(n_emitters), dim3(64), lds_triangles * 5u * 4u, st, s, (const RefitUpdate*)records, n_emitters, lds_triangles);
    ++launches;
  }
  launch_refit_trees(st, s, tlas, tlas_count, orderings, light_lo, light_hi, light_count);
  return launches + (tlas_count ? 1u : 0u) + (light_count ? 1u : 0u);
}

}  // namespace hk
