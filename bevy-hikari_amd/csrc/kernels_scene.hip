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
//
// Exactness: everything per instance is the host builder's arithmetic (scene_builder.cpp) operation for operation -
// the double-precision cofactor inverse rounded once, the 8-corner AABB seeded at zero, 0.5 * |cross| triangle areas
// summed in order, the alias-table construction of mod.rs:320-376 - so a refit scene equals what the host path would
// upload for the same tree shape, bit for bit (tests/test_device_refit.py feeds the oracle exactly that).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>

#include <rocprim/rocprim.hpp>

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
__device__ __forceinline__ float hmin(float a, float b) { return b < a ? b : a; }  // std::min / std::max of the host builder
__device__ __forceinline__ float hmax(float a, float b) { return a < b ? b : a; }
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


// ------------------------------------------------------------------ LBVH rebuild of a flat skip-link BVH (Lauterbach 2009 / Karras 2012)
// hk_rebuild_scene_trees: when motion has degraded a refit tree, a NEW tree over the current leaf boxes is built on the
// device - Morton codes of the box centres, one radix sort (rocPRIM), Karras' parallel hierarchy, boxes bottom-up - and
// written straight into the `bvh` 0.7.1 flatten_custom layout the walk expects: a subtree with L leaves occupies 3L - 2
// consecutive nodes, [navigator of the first child][its subtree][navigator of the second child][its subtree], so the position
// of every node follows from leaf counts alone (no traversal, no stack).  Any binary tree over n shapes has 3n - 2 nodes:
// the new tree fills the old one's storage exactly.  Child order per direction octant = the host's hk_bvh_rethread rule.
struct LbvhBuffers {
  uint32_t n;                   // shapes
  const float4 *box_lo, *box_hi;  // LIGHT: derived from emissives instead
  float* bounds;                // 6 floats: min / max of the box centres (x2)
  uint32_t *codes, *codes_sorted, *ids, *ids_sorted;
  // tree nodes: internal i in [0, n - 1), leaf j as n - 1 + j (j = position in the sorted order)
  uint32_t *parent, *left, *right, *first, *last;  // per internal node (first / last: sorted leaf range it covers)
  uint32_t* leaf_parent;        // per sorted leaf
  float4 *node_lo, *node_hi;    // per tree node (2n - 1)
  uint32_t* arrived;            // per internal node: bottom-up visit counter
  uint8_t* swap;                // per internal node: bit o set = the RIGHT child comes first in ordering o
  uint32_t keep_order0;         // 1: ordering 0 keeps left-before-right (the reference's own flattening of an SAH-built tree)
};
namespace {
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {  // 10 bits -> every third bit
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
template <bool LIGHT>
__device__ __forceinline__ void lbvh_shape_box(const RefitScene& s, const LbvhBuffers& b, uint32_t shape, f3& mn, f3& mx) {
  if (LIGHT) {
    const float4 pr = s.emissives[shape].position_radius;
    mn = F3(pr.x - pr.w, pr.y - pr.w, pr.z - pr.w);
    mx = F3(pr.x + pr.w, pr.y + pr.w, pr.z + pr.w);
  } else {
    mn = xyz(F4(b.box_lo[shape]));
    mx = xyz(F4(b.box_hi[shape]));
  }
}
// common prefix length of the (code, position) keys of sorted leaves i and j; -1 outside the array
__device__ __forceinline__ int lbvh_delta(const uint32_t* __restrict__ codes, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = codes[i], c = codes[j];
  if (a != c) return __clz((int)(a ^ c));
  return 32 + __clz(i ^ j);
}
}  // namespace

template <bool LIGHT>
__global__ __launch_bounds__(1024) void k_lbvh_bounds(RefitScene s, LbvhBuffers b) {  // one workgroup
  __shared__ float red[6][16];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = threadIdx.x; i < b.n; i += 1024u) {
    f3 lo, hi;
    lbvh_shape_box<LIGHT>(s, b, i, lo, hi);
    const float c[3] = {lo.x + hi.x, lo.y + hi.y, lo.z + hi.z};
    for (int k = 0; k < 3; ++k) {
      mn[k] = fminf(mn[k], c[k]);
      mx[k] = fmaxf(mx[k], c[k]);
    }
  }
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    }
  if ((threadIdx.x & 63u) == 0u)
    for (int k = 0; k < 3; ++k) {
      red[k][threadIdx.x >> 6] = mn[k];
      red[3 + k][threadIdx.x >> 6] = mx[k];
    }
  __syncthreads();
  if (threadIdx.x < 6u) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < 16; ++w) v = threadIdx.x < 3u ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    b.bounds[threadIdx.x] = v;
  }
}
template <bool LIGHT>
__global__ __launch_bounds__(256) void k_lbvh_codes(RefitScene s, LbvhBuffers b) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= b.n) return;
  f3 lo, hi;
  lbvh_shape_box<LIGHT>(s, b, i, lo, hi);
  const float c[3] = {lo.x + hi.x, lo.y + hi.y, lo.z + hi.z};
  uint32_t q[3];
  for (int k = 0; k < 3; ++k) {
    const float ext = b.bounds[3 + k] - b.bounds[k];
    const float t = ext > 0.0f ? (c[k] - b.bounds[k]) / ext : 0.0f;
    q[k] = (uint32_t)fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
  }
  b.codes[i] = (expand_bits(q[0]) << 2) | (expand_bits(q[1]) << 1) | expand_bits(q[2]);
  b.ids[i] = i;
}
// Karras 2012, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", section 4: one thread per internal node
__global__ __launch_bounds__(256) void k_lbvh_hierarchy(LbvhBuffers b) {
  const int n = (int)b.n, i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n - 1) return;
  const uint32_t* codes = b.codes_sorted;
  const int d = (lbvh_delta(codes, n, i, i + 1) - lbvh_delta(codes, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = lbvh_delta(codes, n, i, i - d);
  int lmax = 2;
  while (lbvh_delta(codes, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (lbvh_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = lbvh_delta(codes, n, i, j);
  int sft = 0;
  for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (lbvh_delta(codes, n, i, i + (sft + t) * d) > dnode) sft += t;
    if (t <= 1) break;
  }
  const int gamma = i + sft * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  const uint32_t lc = (lo == gamma) ? (uint32_t)(n - 1 + gamma) : (uint32_t)gamma;              // leaf gamma or internal gamma
  const uint32_t rc = (hi == gamma + 1) ? (uint32_t)(n - 1 + gamma + 1) : (uint32_t)(gamma + 1);
  b.left[i] = lc;
  b.right[i] = rc;
  b.first[i] = (uint32_t)lo;
  b.last[i] = (uint32_t)hi;
  if (lc >= (uint32_t)(n - 1)) b.leaf_parent[lc - (uint32_t)(n - 1)] = (uint32_t)i; else b.parent[lc] = (uint32_t)i;
  if (rc >= (uint32_t)(n - 1)) b.leaf_parent[rc - (uint32_t)(n - 1)] = (uint32_t)i; else b.parent[rc] = (uint32_t)i;
  if (i == 0) b.parent[0] = HK_U32_MAX;
}
// leaf boxes, then every internal node by the second of its children to arrive (min / max are exact: any order gives the same box)
template <bool LIGHT>
__global__ __launch_bounds__(256) void k_lbvh_boxes(RefitScene s, LbvhBuffers b) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= b.n) return;
  f3 mn, mx;
  lbvh_shape_box<LIGHT>(s, b, b.ids_sorted[j], mn, mx);
  b.node_lo[b.n - 1u + j] = make_float4(mn.x, mn.y, mn.z, 0.0f);
  b.node_hi[b.n - 1u + j] = make_float4(mx.x, mx.y, mx.z, 0.0f);
  if (b.n == 1u) return;
  uint32_t p = b.leaf_parent[j];
  if (p == HK_U32_MAX) return;  // (a forest build: the only leaf of a one-triangle tree)
  for (;;) {
    __threadfence();
    if (atomicAdd(&b.arrived[p], 1u) == 0u) return;  // the sibling subtree is not finished: its thread continues from here
    __threadfence();
    const uint32_t l = b.left[p], r = b.right[p];
    const volatile float4* vlo = b.node_lo;
    const volatile float4* vhi = b.node_hi;
    const f3 al = F3(vlo[l].x, vlo[l].y, vlo[l].z), ah = F3(vhi[l].x, vhi[l].y, vhi[l].z);
    const f3 bl = F3(vlo[r].x, vlo[r].y, vlo[r].z), bh = F3(vhi[r].x, vhi[r].y, vhi[r].z);
    b.node_lo[p] = make_float4(hmin(al.x, bl.x), hmin(al.y, bl.y), hmin(al.z, bl.z), 0.0f);
    b.node_hi[p] = make_float4(hmax(ah.x, bh.x), hmax(ah.y, bh.y), hmax(ah.z, bh.z), 0.0f);
    // child order per direction octant: host_logic.cpp rethread_flat_bvh (the axis along which the two boxes are furthest apart)
    int axis = 0;
    float best = -1.0f, ca_axis = 0.0f, cb_axis = 0.0f;
    const float ca[3] = {al.x + ah.x, al.y + ah.y, al.z + ah.z}, cb[3] = {bl.x + bh.x, bl.y + bh.y, bl.z + bh.z};
    for (int k = 0; k < 3; ++k) {
      const float dd = fabsf(ca[k] - cb[k]);
      if (dd > best) { best = dd; axis = k; ca_axis = ca[k]; cb_axis = cb[k]; }
    }
    const bool a_lower = ca_axis <= cb_axis;
    uint32_t sw = 0u;
    for (uint32_t o = 0; o < 8u; ++o) {
      const bool negative = (o >> axis) & 1u;
      if (!(a_lower != negative)) sw |= 1u << o;
    }
    if (b.keep_order0) sw &= ~1u;
    b.swap[p] = (uint8_t)sw;
    p = b.parent[p];
    if (p == HK_U32_MAX) return;
  }
}
// every tree node except the root writes the navigator in front of its subtree; leaves also write their own slot
__global__ __launch_bounds__(256) void k_lbvh_emit(LbvhBuffers b, float4* lo, float4* hi, uint32_t stride, size_t ord_stride /* float4 between orderings */, uint32_t orderings) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, n = b.n, total = 2u * n - 1u;
  if (t >= total * orderings) return;
  const uint32_t o = t / total, v = t - o * total;
  float4* nlo = lo + (size_t)o * ord_stride;
  float4* nhi = hi + (size_t)o * ord_stride;
  const bool leaf = v >= n - 1u;
  const uint32_t shape = leaf ? b.ids_sorted[v - (n - 1u)] : 0u;
  const float4 blo = b.node_lo[v], bhi = b.node_hi[v];
  if (n == 1u) {  // flatten_custom of a single leaf: the leaf alone
    nlo[0] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[0] = make_float4(bhi.x, bhi.y, bhi.z, u2f(1u));
    return;
  }
  if (!leaf && v == 0u) return;  // the root has no navigator
  // start of this node's subtree: walk to the root; a first child starts one node after its parent's start (its navigator),
  // a second child after the whole first branch
  auto leaves_of = [&](uint32_t node) { return node >= n - 1u ? 1u : b.last[node] - b.first[node] + 1u; };
  uint32_t start = 0u, c = v, p = leaf ? b.leaf_parent[v - (n - 1u)] : b.parent[v];
  while (p != HK_U32_MAX) {
    const bool right_first = (b.swap[p] >> o) & 1u;
    const uint32_t first_child = right_first ? b.right[p] : b.left[p];
    start += (c == first_child) ? 1u : 2u + (3u * leaves_of(first_child) - 2u);
    c = p;
    p = b.parent[p];
  }
  const uint32_t size = 3u * leaves_of(v) - 2u;
  if (leaf) {  // folded navigator (context.hip fold_leaf_navigators) + the leaf slot
    nlo[(size_t)(start - 1u) * stride] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[(size_t)(start - 1u) * stride] = make_float4(bhi.x, bhi.y, bhi.z, u2f(start + 1u));
    nlo[(size_t)start * stride] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[(size_t)start * stride] = make_float4(bhi.x, bhi.y, bhi.z, u2f(start + 1u));
  } else {
    nlo[(size_t)(start - 1u) * stride] = make_float4(blo.x, blo.y, blo.z, u2f(start));
    nhi[(size_t)(start - 1u) * stride] = make_float4(bhi.x, bhi.y, bhi.z, u2f(start + size));
  }
}


// ------------------------------------------------------------------ the reference's own tree, built on the device
// `bvh` 0.7.1 BVHNode::build (scene_builder.cpp build_recursive; the crate the reference calls at instance.rs:365-371,422-428) is a
// top-down binned SAH: per node the bounds of the shapes and of their centres, the longest axis of the centre bounds, six buckets
// along it, the cheapest of the five splits, the shapes re-ordered bucket by bucket.  Every reduction in it is a min, a max or a
// count, and the re-ordering is a STABLE sort by bucket: nothing depends on the order in which a parallel machine visits the
// shapes.  So the same tree can be built level by level: one workgroup, all nodes of a level at once, the shapes in one array
// that is stably re-sorted per level (block scans of the six bucket flags, segmented at node boundaries, with running counters
// per node and bucket across the 1024-item chunks).  The costs are the host's float expressions term for term, so the splits -
// and with them the shape of the tree - are the host's: tests compare the entry / exit links with the host builder's arrays.
// (Zeros may come out with the other sign than std::min / std::max chains give - a box bound of -0 vs +0 changes no decision.)
struct SahBuffers {
  uint32_t* order[2];      // shape ids, segment by segment
  uint32_t* item_node[2];  // per position: the internal node whose segment it is in, or SAH_DONE once it is a leaf
  uint8_t* item_bucket;
  uint32_t* active[2];     // internal nodes split at this level / created for the next
  uint32_t* acc;           // per internal node: 54 words - bounds (6), centre bounds (6), 6 bucket boxes (36), 6 bucket counts
  float* split;            // per internal node: 4 words - centre-bounds min on the axis, axis size, (bits) axis, (bits) half-split flag
  uint32_t* offsets;       // per internal node: 14 words - first target position of each bucket (6), running counts (6), left count, split bucket
  uint32_t* node_level;    // per internal node: the level of the loop that splits it
  uint32_t* roots;         // nodes handed to k_sah_subtrees
  uint32_t* counters;      // [0] internal nodes allocated, [1] subtree roots, [2] the ping-pong side the top of the tree ended on
};
namespace {
constexpr uint32_t SAH_DONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t fkey(float f) {  // monotone map f32 -> u32 (for atomicMin / atomicMax)
  const uint32_t u = f2u(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ float box_center(float mn, float mx) { return mn + (mx - mn) / 2.0f; }  // Box::center
__device__ __forceinline__ float box_area(const float* mn, const float* mx) {                      // Box::surface_area
  const float x = mx[0] - mn[0], y = mx[1] - mn[1], z = mx[2] - mn[2];
  return 2.0f * (x * y + x * z + y * z);
}
// min / max of a box into the accumulator words acc[0..5] (keys): when every lane of the wave that takes part adds to the SAME
// accumulator (the top levels of the tree: thousands of shapes per node) the wave reduces first - one hot address takes ~10 ns per
// atomic - otherwise every lane adds on its own.  Called by all lanes of the wave; `take` = this lane has a box for `acc`.
__device__ __forceinline__ void wave_box_accumulate(uint32_t* acc, bool take, const float* mn, const float* mx, uint32_t* count) {
  const unsigned long long m = __ballot(take);
  if (m == 0ull) return;
  const unsigned long long a = (unsigned long long)(size_t)acc;
  const int leader = __ffsll((long long)m) - 1;
  const unsigned long long a0 = __shfl(a, leader);
  const bool uniform = __ballot(take && a != a0) == 0ull;
  if (uniform) {
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
      lo[k] = take ? mn[k] : INFINITY;
      hi[k] = take ? mx[k] : -INFINITY;
      for (int off = 32; off > 0; off >>= 1) {
        lo[k] = fminf(lo[k], __shfl_xor(lo[k], off));
        hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off));
      }
    }
    if ((int)(threadIdx.x & 63u) == leader) {
      for (int k = 0; k < 3; ++k) {
        atomicMin(&acc[k], fkey(lo[k]));
        atomicMax(&acc[3 + k], fkey(hi[k]));
      }
      if (count) atomicAdd(count, (uint32_t)__popcll(m));
    }
  } else if (take) {
    for (int k = 0; k < 3; ++k) {
      atomicMin(&acc[k], fkey(mn[k]));
      atomicMax(&acc[3 + k], fkey(mx[k]));
    }
    if (count) atomicAdd(count, 1u);
  }
}
// the six bucket-flag prefix sums (packed two 16-bit counters per word: a chunk has 1024 items) and the run-head maximum of a chunk
// in ONE pass: three block barriers instead of twenty-one.  lds: 4 x 17 words
__device__ __forceinline__ void block_scan_buckets_and_heads(uint32_t bk, uint32_t head_value, uint32_t* lds, uint32_t pre[3], uint32_t& head) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t v[3] = {0u, 0u, 0u};
  if (bk < 6u) v[bk >> 1] = 1u << (16u * (bk & 1u));
  uint32_t inc[3] = {v[0], v[1], v[2]}, hmax = head_value;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t0 = __shfl_up(inc[0], off), t1 = __shfl_up(inc[1], off), t2 = __shfl_up(inc[2], off), th = __shfl_up(hmax, off);
    if ((int)lane >= off) {
      inc[0] += t0;
      inc[1] += t1;
      inc[2] += t2;
      hmax = max(hmax, th);
    }
  }
  __syncthreads();
  if (lane == 63u) {
    lds[wave] = inc[0];
    lds[17 + wave] = inc[1];
    lds[34 + wave] = inc[2];
    lds[51 + wave] = hmax;
  }
  __syncthreads();
  if (threadIdx.x < 4u) {
    uint32_t* a = lds + 17u * threadIdx.x;
    uint32_t run = 0u;
    for (int w = 0; w < 16; ++w) {
      const uint32_t t = a[w];
      a[w] = run;
      run = threadIdx.x == 3u ? max(run, t) : run + t;
    }
  }
  __syncthreads();
  for (int k = 0; k < 3; ++k) pre[k] = lds[17 * k + wave] + inc[k] - v[k];
  head = max(lds[51 + wave], hmax);
}
// step C of a level: the split axis of `node` from its centre bounds (Box::largest_axis), and whether its shapes are too close together
__device__ __forceinline__ void sah_split_axis(const SahBuffers& q, uint32_t node) {
  const uint32_t* acc = q.acc + (size_t)node * 54u;
  float cmn[3], cmx[3];
  for (int k = 0; k < 3; ++k) {
    cmn[k] = funkey(acc[6 + k]);
    cmx[k] = funkey(acc[9 + k]);
  }
  const float x = cmx[0] - cmn[0], y = cmx[1] - cmn[1], z = cmx[2] - cmn[2];
  const int axis = (x > y && x > z) ? 0 : (y > z ? 1 : 2);  // Box::largest_axis
  const float axis_size = cmx[axis] - cmn[axis];
  float* sp = q.split + (size_t)node * 4u;
  sp[0] = cmn[axis];
  sp[1] = axis_size;
  sp[2] = u2f((uint32_t)axis);
  sp[3] = u2f(axis_size < 0.00001f ? 1u : 0u);  // shapes too close together: the index list is cut in half
}
// step E of a level: the cheapest of the five splits of `node` (the host's float expressions term for term), its bucket offsets and its
// children - `child` receives their tree nodes.  A child to split at the next level is appended to active_out[*n_out]
__device__ __forceinline__ void sah_split_node(const LbvhBuffers& b, const SahBuffers& q, uint32_t node, uint32_t level, uint32_t defer, uint32_t* active_out,
                                               uint32_t* n_out, uint32_t child[2]) {
  const uint32_t n = b.n;
  const uint32_t* acc = q.acc + (size_t)node * 54u;
  const float* sp = q.split + (size_t)node * 4u;
  uint32_t* off = q.offsets + (size_t)node * 14u;
  const uint32_t begin = b.first[node], count = b.last[node] - begin + 1u;
  uint32_t n_left = count / 2u, split_bucket = 6u;  // 6: cut the list in half
  if (f2u(sp[3]) == 0u) {
    float bounds_mn[3], bounds_mx[3];
    for (int k = 0; k < 3; ++k) {
      bounds_mn[k] = funkey(acc[k]);
      bounds_mx[k] = funkey(acc[3 + k]);
    }
    const float total_area = box_area(bounds_mn, bounds_mx);
    float min_cost = INFINITY;
    uint32_t min_bucket = 0u;
    for (uint32_t i = 0; i < 5u; ++i) {
      float lmn[3] = {INFINITY, INFINITY, INFINITY}, lmx[3] = {-INFINITY, -INFINITY, -INFINITY};
      float rmn[3] = {INFINITY, INFINITY, INFINITY}, rmx[3] = {-INFINITY, -INFINITY, -INFINITY};
      uint32_t ln = 0u, rn = 0u;
      for (uint32_t k6 = 0; k6 < 6u; ++k6) {
        const uint32_t* bb = acc + 12u + 6u * k6;
        float* tmn = k6 <= i ? lmn : rmn;
        float* tmx = k6 <= i ? lmx : rmx;
        for (int k = 0; k < 3; ++k) {
          tmn[k] = hmin(tmn[k], funkey(bb[k]));
          tmx[k] = hmax(tmx[k], funkey(bb[3 + k]));
        }
        if (k6 <= i) ln += acc[48u + k6]; else rn += acc[48u + k6];
      }
      const float cost = ((float)ln * box_area(lmn, lmx) + (float)rn * box_area(rmn, rmx)) / total_area;
      if (cost < min_cost) {
        min_bucket = i;
        min_cost = cost;
      }
    }
    uint32_t best_left = 0u;  // (all costs NaN: the host keeps bucket 0 as the split)
    for (uint32_t k6 = 0; k6 <= min_bucket; ++k6) best_left += acc[48u + k6];
    if (best_left != 0u && best_left != count) {
      n_left = best_left;
      split_bucket = min_bucket;
    }  // (an empty side - NaN costs - falls back to the half cut, like the host)
  }
  uint32_t run = begin;
  for (uint32_t k6 = 0; k6 < 6u; ++k6) {
    off[k6] = run;
    run += acc[48u + k6];
    off[6u + k6] = 0u;
  }
  off[12] = n_left;
  off[13] = split_bucket;
  // children: a side with one shape is a leaf at its position, a larger one an internal node - split at the next level, or
  // handed to a workgroup of its own when it is small enough
  const uint32_t n_right = count - n_left;
  for (int side = 0; side < 2; ++side) {
    const uint32_t c_begin = side == 0 ? begin : begin + n_left, c_count = side == 0 ? n_left : n_right;
    if (c_count == 1u) {
      child[side] = (n - 1u) + c_begin;
      b.leaf_parent[c_begin] = node;
    } else {
      const uint32_t id = atomicAdd(&q.counters[0], 1u);
      child[side] = id;
      b.first[id] = c_begin;
      b.last[id] = c_begin + c_count - 1u;
      b.parent[id] = node;
      if (c_count <= defer) {
        q.node_level[id] = SAH_DONE;  // (not a level of this loop)
        q.roots[atomicAdd(&q.counters[1], 1u)] = id;
      } else {
        q.node_level[id] = level + 1u;
        active_out[atomicAdd(n_out, 1u)] = id;
      }
    }
  }
  b.left[node] = child[0];
  b.right[node] = child[1];
}
}  // namespace

// The level loop over one range [r0, r1) of item positions, run by ONE workgroup of 1024 threads: every node of a level at once.
// `first_level`: node_level value of the range's root (the nodes created below get first_level + 1, ...).  Nodes with at most
// `defer` shapes are not split here but appended to q.roots (their subtrees are built by k_sah_subtrees, one workgroup each, all
// at once).  Returns the ping-pong side that holds the range's final order.
template <bool LIGHT>
__device__ uint32_t sah_levels(const RefitScene& s, const LbvhBuffers& b, const SahBuffers& q, uint32_t r0, uint32_t r1, uint32_t root, uint32_t cur, uint32_t first_level,
                               uint32_t defer) {
  __shared__ uint32_t scan_lds[68];
  __shared__ uint16_t pre[6][1024];  // per chunk: exclusive prefix of each bucket's flags
  __shared__ uint32_t head_of[1024];
  __shared__ uint32_t n_active_lds[2];
  const uint32_t n = b.n, tid = threadIdx.x;
  if (tid == 0u) {
    q.active[cur][r0] = root;
    q.node_level[root] = first_level;
    n_active_lds[cur] = 1u;
    n_active_lds[cur ^ 1u] = 0u;
  }
  __syncthreads();
  for (uint32_t level = first_level;; ++level) {  // (a level with nothing to split ends the loop)
    const uint32_t n_active = n_active_lds[cur];
    if (n_active == 0u) break;
    const uint32_t* order = q.order[cur];
    const uint32_t* item_node = q.item_node[cur];
    uint32_t* order_out = q.order[cur ^ 1u];
    uint32_t* item_node_out = q.item_node[cur ^ 1u];
    const uint32_t* active = q.active[cur] + r0;
    uint32_t* active_out = q.active[cur ^ 1u] + r0;
    auto splitting = [&](uint32_t node) { return node != SAH_DONE && q.node_level[node] == level; };
    // A: accumulators
    for (uint32_t a = tid; a < n_active * 54u; a += 1024u) {
      const uint32_t node = active[a / 54u], w = a % 54u;
      uint32_t init = 0u;                                             // counts
      if (w < 48u) init = (w % 6u) < 3u ? fkey(INFINITY) : fkey(-INFINITY);  // a box: min xyz, max xyz
      q.acc[(size_t)node * 54u + w] = init;
    }
    __syncthreads();
    if (tid == 0u) n_active_lds[cur ^ 1u] = 0u;
    // B: bounds of the shapes and of their centres
    for (uint32_t p0 = r0; p0 < r1; p0 += 1024u) {  // (block-uniform trip count: the wave reductions want whole waves)
      const uint32_t p = p0 + tid;
      const uint32_t node = p < r1 ? item_node[p] : SAH_DONE;
      const bool take = splitting(node);
      float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}, cc[3] = {0, 0, 0};
      if (take) {
        f3 lo, hi;
        lbvh_shape_box<LIGHT>(s, b, order[p], lo, hi);
        mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z;
        mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
        for (int k = 0; k < 3; ++k) cc[k] = box_center(mn[k], mx[k]);
      }
      uint32_t* acc = q.acc + (size_t)(take ? node : 0u) * 54u;
      wave_box_accumulate(acc, take, mn, mx, nullptr);
      wave_box_accumulate(acc + 6, take, cc, cc, nullptr);
    }
    __syncthreads();
    // C: split axis
    for (uint32_t a = tid; a < n_active; a += 1024u) sah_split_axis(q, active[a]);
    __syncthreads();
    // D: buckets
    for (uint32_t p0 = r0; p0 < r1; p0 += 1024u) {
      const uint32_t p = p0 + tid;
      const uint32_t node = p < r1 ? item_node[p] : SAH_DONE;
      bool take = splitting(node);
      float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
      int bk = 0;
      if (take) {
        const float* sp = q.split + (size_t)node * 4u;
        take = f2u(sp[3]) == 0u;
        if (take) {
          f3 lo, hi;
          lbvh_shape_box<LIGHT>(s, b, order[p], lo, hi);
          mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z;
          mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
          const int axis = (int)f2u(sp[2]);
          const float rel = (box_center(mn[axis], mx[axis]) - sp[0]) / sp[1];
          bk = (int)(rel * (6.0f - 0.01f));
          bk = min(max(bk, 0), 5);
          q.item_bucket[p] = (uint8_t)bk;
        }
      }
      for (int k6 = 0; k6 < 6; ++k6) {  // bucket by bucket: lanes of one node and one bucket share an accumulator
        const bool mine = take && bk == k6;
        uint32_t* acc = q.acc + (size_t)(mine ? node : 0u) * 54u;
        wave_box_accumulate(acc + 12 + 6 * k6, mine, mn, mx, acc + 48 + k6);
      }
    }
    __syncthreads();
    // E: the cheapest split, the children
    for (uint32_t a = tid; a < n_active; a += 1024u) {
      uint32_t child[2];
      sah_split_node(b, q, active[a], level, defer, active_out, &n_active_lds[cur ^ 1u], child);
    }
    __syncthreads();
    // F: stable re-order, bucket by bucket inside every segment; chunk after chunk so that the running counts stay in order
    for (uint32_t c0 = r0; c0 < r1; c0 += 1024u) {
      const uint32_t p = c0 + tid;
      const bool in = p < r1;
      const uint32_t node = in ? item_node[p] : SAH_DONE;
      const bool split_now = in && splitting(node);
      const bool moving = split_now && q.offsets[(size_t)node * 14u + 13u] != 6u;
      const uint32_t bk = moving ? q.item_bucket[p] : 7u;
      const bool head = tid == 0u || !in || item_node[p - 1u] != node;
      uint32_t packed[3], h;
      block_scan_buckets_and_heads(bk, head ? tid : 0u, scan_lds, packed, h);
      for (uint32_t k6 = 0; k6 < 6u; ++k6) pre[k6][tid] = (uint16_t)((packed[k6 >> 1] >> (16u * (k6 & 1u))) & 0xFFFFu);
      head_of[tid] = h;
      __syncthreads();
      if (split_now) {
        const uint32_t* off = q.offsets + (size_t)node * 14u;
        const uint32_t begin = b.first[node], n_left = off[12];
        uint32_t target = p;
        if (moving) target = off[bk] + off[6u + bk] + ((uint32_t)pre[bk][tid] - (uint32_t)pre[bk][h]);
        const bool goes_left = target < begin + n_left;
        const uint32_t child = goes_left ? b.left[node] : b.right[node];
        order_out[target] = order[p];
        item_node_out[target] = child >= n - 1u ? SAH_DONE : child;
      } else if (in) {  // a leaf already, or a node that waits for a workgroup of its own
        order_out[p] = order[p];
        item_node_out[p] = node;
      }
      __syncthreads();
      // the last item of a node's run in this chunk adds the chunk's counts to the node's running counts
      if (moving) {
        const bool last_of_run = tid == 1023u || p + 1u >= r1 || item_node[p + 1u] != node;
        if (last_of_run) {
          uint32_t* off = q.offsets + (size_t)node * 14u;
          for (uint32_t k6 = 0; k6 < 6u; ++k6) off[6u + k6] += ((uint32_t)pre[k6][tid] + (bk == k6 ? 1u : 0u)) - (uint32_t)pre[k6][h];
        }
      }
      __syncthreads();
    }
    cur ^= 1u;
  }
  __syncthreads();
  return cur;
}

// SAH_SUBTREE: nodes with at most this many shapes are built by a workgroup of their own (k_sah_subtrees), all of them at once
constexpr uint32_t SAH_SUBTREE = 1024u;
// the top of the tree: one workgroup over the whole array, down to nodes of at most SAH_SUBTREE shapes.  Outputs the LbvhBuffers
// topology (ids_sorted = leaf order, parent / left / right / first / last / leaf_parent) for k_lbvh_boxes + k_lbvh_emit
template <bool LIGHT>
__global__ __launch_bounds__(1024) void k_sah_build(RefitScene s, LbvhBuffers b, SahBuffers q) {
  const uint32_t n = b.n, tid = threadIdx.x;
  if (n == 1u) {
    if (tid == 0u) {
      b.ids_sorted[0] = 0u;
      q.counters[1] = 0u;
    }
    return;
  }
  for (uint32_t i = tid; i < n; i += 1024u) {
    q.order[0][i] = i;
    q.item_node[0][i] = 0u;
  }
  if (tid == 0u) {
    b.first[0] = 0u;
    b.last[0] = n - 1u;
    b.parent[0] = HK_U32_MAX;
    q.counters[0] = 1u;  // internal nodes allocated
    q.counters[1] = 0u;  // subtree roots
  }
  __syncthreads();
  const uint32_t cur = sah_levels<LIGHT>(s, b, q, 0u, n, 0u, 0u, 0u, n > SAH_SUBTREE ? SAH_SUBTREE : 0u);
  if (tid == 0u) q.counters[2] = cur;  // the side the subtree workgroups start from
  // leaves fixed at this stage are final; the ranges of the deferred nodes are copied by their own workgroups
  for (uint32_t i = tid; i < n; i += 1024u)
    if (q.item_node[cur][i] == SAH_DONE) b.ids_sorted[i] = q.order[cur][i];
}
// the subtrees below: one workgroup per deferred node, all at once
template <bool LIGHT>
__global__ __launch_bounds__(1024) void k_sah_subtrees(RefitScene s, LbvhBuffers b, SahBuffers q) {
  const uint32_t n_roots = q.counters[1], start = q.counters[2];
  for (uint32_t r = blockIdx.x; r < n_roots; r += gridDim.x) {
    const uint32_t root = q.roots[r], r0 = b.first[root], r1 = b.last[root] + 1u;
    const uint32_t cur = sah_levels<LIGHT>(s, b, q, r0, r1, root, start, 0x40000000u, 0u);
    for (uint32_t i = r0 + threadIdx.x; i < r1; i += 1024u) b.ids_sorted[i] = q.order[cur][i];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ the top of the SAH tree on the whole chip
// k_sah_build runs every level above SAH_SUBTREE-shape nodes in ONE workgroup: sized for 2 * 10^4 instances, not for the 10^5 - 10^6
// triangles of a mesh (hk_rebuild_mesh_tree).  Here a level is five stream-ordered launches over 1024-item chunks, one workgroup per
// chunk - bounds (B), axis (C), buckets (D), split (E), re-order (F) - with sah_levels' arithmetic (sah_split_axis / sah_split_node are
// shared, B / D / F restate its item steps).  What changes is only how the order-free reductions travel:
//   - the segments of the nodes are contiguous, so a chunk whose first and last item share a node belongs to that node alone: its
//     workgroup reduces in LDS (wave_box_accumulate on LDS words) and adds ONE set of atomics per chunk to the node's accumulators -
//     at the top levels that is every chunk, and the hot addresses see a thousand atomics instead of a million;
//   - the stable re-order needs, per item, the count of its bucket in its node BEFORE the chunk.  Only the run at the head of a chunk
//     can have begun earlier, and in each earlier chunk its node is the tail run (first chunk) or the whole chunk: D leaves the six
//     bucket counts of every chunk's head run and tail run in `chunk_counts`, F sums the ones it needs (integers: any order).
// The host launches a FIXED number of levels (it reads nothing back); nodes still unsplit after them go to k_sah_subtrees like the
// small ones, which is correct at any node size.  counters[8 + level] = nodes to split at `level`.
constexpr uint32_t SAH_WIDE_MIN = 32768u;       // shapes from which the top of the tree is built this way
constexpr uint32_t SAH_WIDE_MAX_LEVELS = 48u;   // counters[] holds 64 words
namespace {
__device__ __forceinline__ uint32_t sah_acc_init(uint32_t w) { return w < 48u ? ((w % 6u) < 3u ? fkey(INFINITY) : fkey(-INFINITY)) : 0u; }
__device__ __forceinline__ bool sah_splitting(const SahBuffers& q, uint32_t node, uint32_t level) { return node != SAH_DONE && q.node_level[node] == level; }
}  // namespace
__global__ __launch_bounds__(1024) void k_sahw_setup(LbvhBuffers b, SahBuffers q, uint32_t levels) {
  const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
  if (i < b.n) {
    q.order[0][i] = i;
    q.item_node[0][i] = 0u;
  }
  if (blockIdx.x != 0u) return;
  if (threadIdx.x < 54u) q.acc[threadIdx.x] = sah_acc_init(threadIdx.x);
  if (threadIdx.x < 64u) {
    uint32_t v = 0u;
    if (threadIdx.x == 0u || threadIdx.x == 8u) v = 1u;  // internal nodes allocated; one node to split at level 0
    if (threadIdx.x == 2u) v = levels & 1u;              // the ping-pong side the subtree workgroups start from
    q.counters[threadIdx.x] = v;
  }
  if (threadIdx.x == 0u) {
    b.first[0] = 0u;
    b.last[0] = b.n - 1u;
    b.parent[0] = HK_U32_MAX;
    q.active[0][0] = 0u;
    q.node_level[0] = 0u;
  }
}
// B: bounds of the shapes and of their centres
__global__ __launch_bounds__(1024) void k_sahw_bounds(LbvhBuffers b, SahBuffers q, uint32_t level) {
  __shared__ uint32_t lacc[12];
  const RefitScene none{};
  const uint32_t tid = threadIdx.x, n = b.n, side = level & 1u, c0 = blockIdx.x * 1024u, p = c0 + tid;
  const uint32_t* item_node = q.item_node[side];
  const uint32_t hn = item_node[c0], tn = item_node[min(c0 + 1023u, n - 1u)];
  const bool uniform = hn == tn;
  if (uniform && !sah_splitting(q, hn, level)) return;  // (block-uniform)
  if (tid < 12u) lacc[tid] = sah_acc_init(tid);
  __syncthreads();
  const uint32_t node = p < n ? item_node[p] : SAH_DONE;
  const bool take = sah_splitting(q, node, level);
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}, cc[3] = {0, 0, 0};
  if (take) {
    f3 lo, hi;
    lbvh_shape_box<false>(none, b, q.order[side][p], lo, hi);
    mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z;
    mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
    for (int k = 0; k < 3; ++k) cc[k] = box_center(mn[k], mx[k]);
  }
  uint32_t* acc = uniform ? lacc : q.acc + (size_t)(take ? node : 0u) * 54u;
  wave_box_accumulate(acc, take, mn, mx, nullptr);
  wave_box_accumulate(acc + 6, take, cc, cc, nullptr);
  if (!uniform) return;
  __syncthreads();
  if (tid < 12u) {
    uint32_t* g = q.acc + (size_t)hn * 54u + tid;
    if ((tid % 6u) < 3u) atomicMin(g, lacc[tid]); else atomicMax(g, lacc[tid]);
  }
}
// C: split axis
__global__ __launch_bounds__(256) void k_sahw_axis(SahBuffers q, uint32_t level) {
  const uint32_t n_active = q.counters[8u + level];
  const uint32_t* active = q.active[level & 1u];
  for (uint32_t a = blockIdx.x * 256u + threadIdx.x; a < n_active; a += gridDim.x * 256u) sah_split_axis(q, active[a]);
}
// D: buckets; chunk_counts[12 * chunk ..]: the six bucket counts of the chunk's head run, then of its tail run
__global__ __launch_bounds__(1024) void k_sahw_buckets(LbvhBuffers b, SahBuffers q, uint32_t level, uint32_t* __restrict__ chunk_counts) {
  __shared__ uint32_t lacc[42];  // six bucket boxes, six counts
  __shared__ uint32_t runs[12];
  const RefitScene none{};
  const uint32_t tid = threadIdx.x, n = b.n, side = level & 1u, c0 = blockIdx.x * 1024u, p = c0 + tid;
  const uint32_t* item_node = q.item_node[side];
  const uint32_t hn = item_node[c0], tn = item_node[min(c0 + 1023u, n - 1u)];
  const bool uniform = hn == tn;
  if (uniform && !sah_splitting(q, hn, level)) return;  // (block-uniform; F never reads this chunk's counts)
  if (tid < 42u) lacc[tid] = tid < 36u ? sah_acc_init(tid) : 0u;
  if (tid < 12u) runs[tid] = 0u;
  __syncthreads();
  const uint32_t node = p < n ? item_node[p] : SAH_DONE;
  bool take = sah_splitting(q, node, level);
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  int bk = 0;
  if (take) {
    const float* sp = q.split + (size_t)node * 4u;
    take = f2u(sp[3]) == 0u;
    if (take) {
      f3 lo, hi;
      lbvh_shape_box<false>(none, b, q.order[side][p], lo, hi);
      mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z;
      mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
      const int axis = (int)f2u(sp[2]);
      const float rel = (box_center(mn[axis], mx[axis]) - sp[0]) / sp[1];
      bk = (int)(rel * (6.0f - 0.01f));
      bk = min(max(bk, 0), 5);
      q.item_bucket[p] = (uint8_t)bk;
    }
  }
  for (int k6 = 0; k6 < 6; ++k6) {
    const bool mine = take && bk == k6;
    uint32_t* acc = q.acc + (size_t)(mine ? node : 0u) * 54u;
    wave_box_accumulate(uniform ? lacc + 6 * k6 : acc + 12 + 6 * k6, mine, mn, mx, uniform ? lacc + 36 + k6 : acc + 48 + k6);
    if (!uniform) {
      const unsigned long long mh = __ballot(mine && node == hn), mt = __ballot(mine && node == tn);
      if ((tid & 63u) == 0u) {
        if (mh) atomicAdd(&runs[k6], (uint32_t)__popcll(mh));
        if (mt) atomicAdd(&runs[6 + k6], (uint32_t)__popcll(mt));
      }
    }
  }
  __syncthreads();
  if (uniform && tid < 42u) {
    uint32_t* g = q.acc + (size_t)hn * 54u + 12u + tid;
    if (tid >= 36u) atomicAdd(g, lacc[tid]);
    else if ((tid % 6u) < 3u) atomicMin(g, lacc[tid]);
    else atomicMax(g, lacc[tid]);
  }
  if (tid < 12u) chunk_counts[12u * blockIdx.x + tid] = uniform ? lacc[36u + tid % 6u] : runs[tid];
}
// E: the cheapest split, the children (their accumulators start empty: there is no step A here)
__global__ __launch_bounds__(256) void k_sahw_split(LbvhBuffers b, SahBuffers q, uint32_t level, uint32_t defer) {
  const uint32_t n_active = q.counters[8u + level];
  const uint32_t* active = q.active[level & 1u];
  for (uint32_t a = blockIdx.x * 256u + threadIdx.x; a < n_active; a += gridDim.x * 256u) {
    uint32_t child[2];
    sah_split_node(b, q, active[a], level, defer, q.active[(level + 1u) & 1u], &q.counters[9u + level], child);
    for (int side = 0; side < 2; ++side)
      if (child[side] < b.n - 1u)
        for (uint32_t w = 0; w < 54u; ++w) q.acc[(size_t)child[side] * 54u + w] = sah_acc_init(w);
  }
}
// F: stable re-order, bucket by bucket inside every segment
__global__ __launch_bounds__(1024) void k_sahw_reorder(LbvhBuffers b, SahBuffers q, uint32_t level, const uint32_t* __restrict__ chunk_counts) {
  __shared__ uint32_t scan_lds[68];
  __shared__ uint16_t pre[6][1024];
  __shared__ uint32_t carry[6];  // per bucket: items of the head run's node in the chunks before this one
  const uint32_t tid = threadIdx.x, n = b.n, side = level & 1u, c0 = blockIdx.x * 1024u, p = c0 + tid;
  const uint32_t* order = q.order[side];
  const uint32_t* item_node = q.item_node[side];
  uint32_t* order_out = q.order[side ^ 1u];
  uint32_t* item_node_out = q.item_node[side ^ 1u];
  const bool in = p < n;
  const uint32_t node = in ? item_node[p] : SAH_DONE;
  const uint32_t hn = item_node[c0], tn = item_node[min(c0 + 1023u, n - 1u)];
  if (hn == tn && !sah_splitting(q, hn, level)) {  // (block-uniform) nothing of this chunk is split at this level
    if (in) {
      order_out[p] = order[p];
      item_node_out[p] = node;
    }
    return;
  }
  const bool split_now = in && sah_splitting(q, node, level);
  const bool moving = split_now && q.offsets[(size_t)node * 14u + 13u] != 6u;
  const uint32_t bk = moving ? q.item_bucket[p] : 7u;
  const bool head = tid == 0u || !in || item_node[p - 1u] != node;
  uint32_t packed[3], h;
  block_scan_buckets_and_heads(bk, head ? tid : 0u, scan_lds, packed, h);
  for (uint32_t k6 = 0; k6 < 6u; ++k6) pre[k6][tid] = (uint16_t)((packed[k6 >> 1] >> (16u * (k6 & 1u))) & 0xFFFFu);
  if (tid < 6u) carry[tid] = 0u;
  __syncthreads();
  if (sah_splitting(q, hn, level) && q.offsets[(size_t)hn * 14u + 13u] != 6u) {  // (block-uniform)
    const uint32_t begin = b.first[hn];
    if (begin < c0 && tid < 1020u) {
      const uint32_t f = begin >> 10, k6 = tid % 6u, g = tid / 6u;  // the node's first chunk: there it is the tail run
      uint32_t sum = g == 0u ? chunk_counts[12u * f + 6u + k6] : 0u;
      for (uint32_t c = f + 1u + g; c < blockIdx.x; c += 170u) sum += chunk_counts[12u * c + k6];  // ... and every chunk between is its alone
      if (sum) atomicAdd(&carry[k6], sum);
    }
  }
  __syncthreads();
  if (split_now) {
    const uint32_t* off = q.offsets + (size_t)node * 14u;
    const uint32_t begin = b.first[node], n_left = off[12];
    uint32_t target = p;
    if (moving) target = off[bk] + (h == 0u ? carry[bk] : 0u) + ((uint32_t)pre[bk][tid] - (uint32_t)pre[bk][h]);
    const bool goes_left = target < begin + n_left;
    const uint32_t child = goes_left ? b.left[node] : b.right[node];
    order_out[target] = order[p];
    item_node_out[target] = child >= n - 1u ? SAH_DONE : child;
  } else if (in) {  // a leaf already, or a node that waits for a workgroup of its own
    order_out[p] = order[p];
    item_node_out[p] = node;
  }
}
// after the last level: the nodes still unsplit join the deferred ones; leaves fixed so far are final
__global__ __launch_bounds__(256) void k_sahw_finish(LbvhBuffers b, SahBuffers q, uint32_t levels) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, side = levels & 1u;
  const uint32_t n_left = q.counters[8u + levels];
  for (uint32_t a = i; a < n_left; a += gridDim.x * 256u) q.roots[atomicAdd(&q.counters[1], 1u)] = q.active[side][a];
  if (i < b.n && q.item_node[side][i] == SAH_DONE) b.ids_sorted[i] = q.order[side][i];
}

// ------------------------------------------------------------------ a FOREST of mesh trees in one build (hk_load_scene)
// A scene arrives with thousands of small meshes: one tree build per mesh is six to forty launches each.  Here the triangles of all the
// meshes of a batch form ONE shape array (mesh m owns the positions [tri_begin, tri_begin + n_tris)), and the trees share the arrays of a
// single build: tree nodes are numbered in one space (internal nodes below n - 1, the leaf at position j is n - 1 + j, n = all the
// triangles of the batch), every mesh's root has no parent, and nothing ever crosses a mesh boundary because a node's segment never
// does.  The binned-SAH trees are sah_levels' - the root of mesh m is internal node m; a mesh above SAH_SUBTREE triangles has its top
// levels split by a workgroup of its own (k_forest_tops), then ALL nodes of at most SAH_SUBTREE triangles, whole small meshes among
// them, are built by k_sah_subtrees at once.  The Morton-order trees sort all meshes' codes in one segmented sort.  Boxes bottom-up are
// k_lbvh_boxes; k_forest_emit is k_lbvh_emit with the mesh's own node range as the target and the triangle index local to the mesh.
// The number of launches depends on the mode, not on the number of meshes.
constexpr uint32_t FOREST_UNUSED = 0xFEFEFEFEu;  // parent[] of an internal node id no tree uses: the array is filled with the BYTE 0xFE
namespace {
__device__ __forceinline__ float forest_leaf_min(float a, float b) {  // kernels_deform.hip leaf_min: IEEE minNum with -0 < +0
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? a : b;
  return a < b ? a : b;
}
__device__ __forceinline__ float forest_leaf_max(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? b : a;
  return a > b ? a : b;
}
}  // namespace
// one workgroup per mesh: the triangle boxes (k_mesh_triangle_boxes' arithmetic), the identity order, the mesh of every position, the root
__global__ __launch_bounds__(256) void k_forest_setup(const ForestMesh* __restrict__ meshes, uint32_t n_meshes, const float4* __restrict__ v0, const float4* __restrict__ v1,
                                                      const float4* __restrict__ v2, float4* __restrict__ tri_lo, float4* __restrict__ tri_hi, uint32_t* __restrict__ item_mesh,
                                                      LbvhBuffers b, SahBuffers q, uint32_t sah) {
  const uint32_t m = blockIdx.x;
  if (m >= n_meshes) return;
  const ForestMesh fm = meshes[m];
  for (uint32_t i = threadIdx.x; i < fm.n_tris; i += 256u) {
    const uint32_t pos = fm.tri_begin + i;
    const float4 a = v0[fm.primitive + i], c = v1[fm.primitive + i], d = v2[fm.primitive + i];
    tri_lo[pos] = make_float4(forest_leaf_min(a.x, forest_leaf_min(c.x, d.x)), forest_leaf_min(a.y, forest_leaf_min(c.y, d.y)), forest_leaf_min(a.z, forest_leaf_min(c.z, d.z)), 0.0f);
    tri_hi[pos] = make_float4(forest_leaf_max(a.x, forest_leaf_max(c.x, d.x)), forest_leaf_max(a.y, forest_leaf_max(c.y, d.y)), forest_leaf_max(a.z, forest_leaf_max(c.z, d.z)), 0.0f);
    item_mesh[pos] = m;
    if (sah) {
      q.order[0][pos] = pos;
      q.item_node[0][pos] = fm.n_tris > 1u ? m : SAH_DONE;
    }
    if (fm.n_tris == 1u) {  // a tree of one leaf: nothing to build
      b.ids_sorted[pos] = pos;
      b.leaf_parent[pos] = HK_U32_MAX;
    }
  }
  if (!sah || threadIdx.x != 0u) return;
  if (m == 0u) q.counters[0] = n_meshes;  // internal nodes allocated: the roots (counters[1], [2] were zeroed by the host)
  if (fm.n_tris > 1u) {
    b.first[m] = fm.tri_begin;
    b.last[m] = fm.tri_begin + fm.n_tris - 1u;
    b.parent[m] = HK_U32_MAX;
    if (fm.n_tris <= SAH_SUBTREE) {
      q.node_level[m] = SAH_DONE;
      q.roots[atomicAdd(&q.counters[1], 1u)] = m;
    }
  }
}
// the top levels of every mesh above SAH_SUBTREE triangles, one workgroup each (k_sah_build's part); the range ends on ping-pong side 0,
// where k_sah_subtrees starts from
__global__ __launch_bounds__(1024) void k_forest_tops(const ForestMesh* __restrict__ meshes, const uint32_t* __restrict__ tops, LbvhBuffers b, SahBuffers q) {
  const RefitScene none{};
  const uint32_t m = tops[blockIdx.x];
  const ForestMesh fm = meshes[m];
  const uint32_t r0 = fm.tri_begin, r1 = fm.tri_begin + fm.n_tris;
  const uint32_t cur = sah_levels<false>(none, b, q, r0, r1, m, 0u, 0u, SAH_SUBTREE);
  for (uint32_t i = r0 + threadIdx.x; i < r1; i += 1024u) {
    const uint32_t node = q.item_node[cur][i], shape = q.order[cur][i];
    if (cur != 0u) {
      q.item_node[0][i] = node;
      q.order[0][i] = shape;
    }
    if (node == SAH_DONE) b.ids_sorted[i] = shape;  // leaves fixed at this stage are final
  }
}
// Morton-order trees: the centre bounds of every mesh (one workgroup each), the codes inside them, Karras' hierarchy per segment
__global__ __launch_bounds__(256) void k_forest_lbvh_bounds(const ForestMesh* __restrict__ meshes, LbvhBuffers b, float* __restrict__ mesh_bounds) {
  __shared__ float red[6][4];
  const ForestMesh fm = meshes[blockIdx.x];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = threadIdx.x; i < fm.n_tris; i += 256u) {
    const float4 lo = b.box_lo[fm.tri_begin + i], hi = b.box_hi[fm.tri_begin + i];
    const float c[3] = {lo.x + hi.x, lo.y + hi.y, lo.z + hi.z};
    for (int k = 0; k < 3; ++k) {
      mn[k] = fminf(mn[k], c[k]);
      mx[k] = fmaxf(mx[k], c[k]);
    }
  }
  for (int k = 0; k < 3; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
      mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
    }
  if ((threadIdx.x & 63u) == 0u)
    for (int k = 0; k < 3; ++k) {
      red[k][threadIdx.x >> 6] = mn[k];
      red[3 + k][threadIdx.x >> 6] = mx[k];
    }
  __syncthreads();
  if (threadIdx.x < 6u) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < 4; ++w) v = threadIdx.x < 3u ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    mesh_bounds[6u * blockIdx.x + threadIdx.x] = v;
  }
}
__global__ __launch_bounds__(256) void k_forest_lbvh_codes(const uint32_t* __restrict__ item_mesh, const float* __restrict__ mesh_bounds, LbvhBuffers b) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= b.n) return;
  const float* bounds = mesh_bounds + 6u * item_mesh[i];
  const float4 lo = b.box_lo[i], hi = b.box_hi[i];
  const float c[3] = {lo.x + hi.x, lo.y + hi.y, lo.z + hi.z};
  uint32_t qv[3];
  for (int k = 0; k < 3; ++k) {
    const float ext = bounds[3 + k] - bounds[k];
    const float t = ext > 0.0f ? (c[k] - bounds[k]) / ext : 0.0f;
    qv[k] = (uint32_t)fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
  }
  b.codes[i] = (expand_bits(qv[0]) << 2) | (expand_bits(qv[1]) << 1) | expand_bits(qv[2]);
  b.ids[i] = i;
}
// k_lbvh_hierarchy inside the segment of the position's mesh: internal node i of a mesh is tree node tri_begin + i
__global__ __launch_bounds__(256) void k_forest_lbvh_hierarchy(const ForestMesh* __restrict__ meshes, const uint32_t* __restrict__ item_mesh, LbvhBuffers b) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= b.n) return;
  const ForestMesh fm = meshes[item_mesh[g]];
  const int n = (int)fm.n_tris, i = (int)(g - fm.tri_begin);
  if (i >= n - 1) return;
  const uint32_t base = fm.tri_begin, leaf0 = b.n - 1u + fm.tri_begin;
  const uint32_t* codes = b.codes_sorted + base;
  const int d = (lbvh_delta(codes, n, i, i + 1) - lbvh_delta(codes, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = lbvh_delta(codes, n, i, i - d);
  int lmax = 2;
  while (lbvh_delta(codes, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (lbvh_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = lbvh_delta(codes, n, i, j);
  int sft = 0;
  for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (lbvh_delta(codes, n, i, i + (sft + t) * d) > dnode) sft += t;
    if (t <= 1) break;
  }
  const int gamma = i + sft * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  const bool l_leaf = lo == gamma, r_leaf = hi == gamma + 1;
  const uint32_t lc = l_leaf ? leaf0 + (uint32_t)gamma : base + (uint32_t)gamma;
  const uint32_t rc = r_leaf ? leaf0 + (uint32_t)gamma + 1u : base + (uint32_t)gamma + 1u;
  b.left[g] = lc;
  b.right[g] = rc;
  b.first[g] = base + (uint32_t)lo;
  b.last[g] = base + (uint32_t)hi;
  if (l_leaf) b.leaf_parent[base + (uint32_t)gamma] = g; else b.parent[lc] = g;
  if (r_leaf) b.leaf_parent[base + (uint32_t)gamma + 1u] = g; else b.parent[rc] = g;
  if (i == 0) b.parent[g] = HK_U32_MAX;
}
// k_lbvh_emit for a forest: every tree node except the roots writes the navigator in front of its subtree into ITS mesh's node range,
// links local to that range; leaves also write their own slot.  parent[] was filled with FOREST_UNUSED before the build
__global__ __launch_bounds__(256) void k_forest_emit(const ForestMesh* __restrict__ meshes, const uint32_t* __restrict__ item_mesh, LbvhBuffers b, float4* nodes,
                                                     size_t ord_stride /* float4 between orderings */, uint32_t orderings) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, n = b.n, total = 2u * n - 1u;
  if (t >= total * orderings) return;
  const uint32_t o = t / total, v = t - o * total;
  const bool leaf = v >= n - 1u;
  uint32_t p;
  if (leaf) {
    p = b.leaf_parent[v - (n - 1u)];
  } else {
    p = b.parent[v];
    if (p == FOREST_UNUSED || p == HK_U32_MAX) return;  // no such node; a root has no navigator
  }
  const ForestMesh fm = meshes[item_mesh[leaf ? v - (n - 1u) : b.first[v]]];
  float4* nlo = nodes + (size_t)o * ord_stride + 2u * (size_t)fm.node_offset;
  float4* nhi = nlo + 1;
  const uint32_t shape = leaf ? b.ids_sorted[v - (n - 1u)] - fm.tri_begin : 0u;
  const float4 blo = b.node_lo[v], bhi = b.node_hi[v];
  if (fm.n_tris == 1u) {  // flatten_custom of a single leaf: the leaf alone
    nlo[0] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[0] = make_float4(bhi.x, bhi.y, bhi.z, u2f(1u));
    return;
  }
  auto leaves_of = [&](uint32_t node) { return node >= n - 1u ? 1u : b.last[node] - b.first[node] + 1u; };
  uint32_t start = 0u, c = v;
  while (p < n - 1u) {  // (up to the root, whose parent is HK_U32_MAX)
    const bool right_first = (b.swap[p] >> o) & 1u;
    const uint32_t first_child = right_first ? b.right[p] : b.left[p];
    start += (c == first_child) ? 1u : 2u + (3u * leaves_of(first_child) - 2u);
    c = p;
    p = b.parent[p];
  }
  const uint32_t size = 3u * leaves_of(v) - 2u;
  if (start == 0u || start > 3u * fm.n_tris - 2u - size) return;  // (never outside the mesh's own range, whatever the arrays hold)
  if (leaf) {  // folded navigator (scene_layout.hip fold_leaf_navigators) + the leaf slot
    nlo[2u * (size_t)(start - 1u)] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[2u * (size_t)(start - 1u)] = make_float4(bhi.x, bhi.y, bhi.z, u2f(start + 1u));
    nlo[2u * (size_t)start] = make_float4(blo.x, blo.y, blo.z, u2f(HK_LEAF | shape));
    nhi[2u * (size_t)start] = make_float4(bhi.x, bhi.y, bhi.z, u2f(start + 1u));
  } else {
    nlo[2u * (size_t)(start - 1u)] = make_float4(blo.x, blo.y, blo.z, u2f(start));
    nhi[2u * (size_t)(start - 1u)] = make_float4(bhi.x, bhi.y, bhi.z, u2f(start + size));
  }
}

// ------------------------------------------------------------------ a deformed mesh's new box, carried to its instances
// One thread per instance of the mesh: the mesh box (order-preserving words of kernels_deform.hip k_mesh_*) as bevy's Aabb, the world
// AABB and emitter record with k_refit_instances' arithmetic (instance_world_box, emitter_position_radius: keep both in step) - but the pose, its previous model and its `moved` flag stay as they are
// (a deformation is no motion: velocity_uv keeps the reference's formula).  Emitters (the first n_emitters ids) also get an update
// record for k_refit_emitters: their triangle areas and alias table follow the new triangles.
__device__ __forceinline__ float mesh_box_word(uint32_t e) { return u2f((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }
__global__ __launch_bounds__(64) void k_mesh_instances(RefitScene s, const uint32_t* __restrict__ box, const uint32_t* __restrict__ ids, uint32_t n_ids,
                                                       RefitUpdate* __restrict__ records, uint32_t n_emitters) {
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= n_ids) return;
  const uint32_t id = ids[u];
  const DInstance& d = s.instances[id];
  const float m[16] = {d.m0.x, d.m0.y, d.m0.z, d.m0.w, d.m1.x, d.m1.y, d.m1.z, d.m1.w, d.m2.x, d.m2.y, d.m2.z, d.m2.w, d.m3.x, d.m3.y, d.m3.z, d.m3.w};
  float ac[3], ah[3];
  for (int k = 0; k < 3; ++k) {  // bevy Aabb::from_min_max (scene_builder.cpp hk_scene_builder_add_mesh)
    const float mn = mesh_box_word(box[k]), mx = mesh_box_word(box[3 + k]);
    ac[k] = 0.5f * (mx + mn);
    ah[k] = 0.5f * (mx - mn);
  }
  float mn[3], mx[3];
  instance_world_box(m, ac, ah, mn, mx);
  s.inst_lo[id] = make_float4(mn[0], mn[1], mn[2], 0.0f);
  s.inst_hi[id] = make_float4(mx[0], mx[1], mx[2], 0.0f);
  if (u >= n_emitters) return;
  const uint32_t e = s.emissive_of_instance[id];
  if (e == HK_U32_MAX) return;
  s.emissives[e].position_radius = emitter_position_radius(s.materials[4u * d.material + 1u], mn, mx);
  RefitUpdate r;
  r.instance = id;
  r.moved = 1u;
  for (int k = 0; k < 16; ++k) r.model[k] = m[k];
  for (int k = 0; k < 3; ++k) {
    r.aabb_center[k] = ac[k];
    r.aabb_half[k] = ah[k];
  }
  records[u] = r;
}

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

}  // namespace hkd

namespace hk {
using namespace hkd;

void launch_material_update(hipStream_t st, const RefitScene& s, float4* materials, const MaterialUpdate* updates, uint32_t n_updates, const uint32_t* emitters,
                            uint32_t n_emitters, float4* light_lo, float4* light_hi, uint32_t light_count) {
  if (n_updates) hipLaunchKernelGGL(k_write_materials, dim3((n_updates + 63u) / 64u), dim3(64), 0, st, materials, updates, n_updates);
  if (!n_emitters) return;
  hipLaunchKernelGGL(k_material_emitters, dim3((n_emitters + 63u) / 64u), dim3(64), 0, st, s, emitters, n_emitters);
  if (light_count) hipLaunchKernelGGL((k_refit_flat_bvh<true>), dim3((light_count + 3u) / 4u), dim3(256), 0, st, s, light_lo, light_hi, 1u, light_count, 1u);
}
void launch_texture_update(hipStream_t st, uint32_t* dst, const uint32_t* src, size_t n, uint4* info0, uint4* info1, uint4 info) {
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 4096));
  hipLaunchKernelGGL(k_update_texture, dim3(blocks), dim3(256), 0, st, dst, src, n, info0, info1, info);
}

void launch_copy_region(hipStream_t st, void* dst, const void* src, size_t bytes) {
  const size_t n = bytes / 16;
  if (!n) return;
  hipLaunchKernelGGL(k_copy_region_u4, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, (uint4*)dst, (const uint4*)src, n);
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
  // TLAS nodes are interleaved (lo, hi) pairs, the light BVH two planes
  if (tlas_count) {
    const uint32_t waves = tlas_count * orderings;
    hipLaunchKernelGGL((k_refit_flat_bvh<false>), dim3((waves + 3u) / 4u), dim3(256), 0, st, s, tlas, tlas + 1, 2u, tlas_count, orderings);
  }
  if (light_count) hipLaunchKernelGGL((k_refit_flat_bvh<true>), dim3((light_count + 3u) / 4u), dim3(256), 0, st, s, light_lo, light_hi, 1u, light_count, 1u);
}

void launch_mesh_propagate(hipStream_t st, const RefitScene& s, const uint32_t* box, const uint32_t* ids, uint32_t n_ids, RefitUpdate* records, uint32_t n_emitters,
                           uint32_t emitter_triangles, float4* tlas, uint32_t tlas_count, uint32_t orderings, float4* light_lo, float4* light_hi, uint32_t light_count) {
  if (n_ids) hipLaunchKernelGGL(k_mesh_instances, dim3((n_ids + 63u) / 64u), dim3(64), 0, st, s, box, ids, n_ids, records, n_emitters);
  if (n_emitters) {
    const uint32_t lds_triangles = std::min(emitter_triangles, HK_EMITTER_LDS_TRIANGLES);
    hipLaunchKernelGGL(k_refit_emitters, dim3(n_emitters), dim3(64), lds_triangles * 5u * 4u, st, s, (const RefitUpdate*)records, n_emitters, lds_triangles);
  }
  if (tlas_count) {
    const uint32_t waves = tlas_count * orderings;
    hipLaunchKernelGGL((k_refit_flat_bvh<false>), dim3((waves + 3u) / 4u), dim3(256), 0, st, s, tlas, tlas + 1, 2u, tlas_count, orderings);
  }
  if (light_count) hipLaunchKernelGGL((k_refit_flat_bvh<true>), dim3((light_count + 3u) / 4u), dim3(256), 0, st, s, light_lo, light_hi, 1u, light_count, 1u);
}
// the refit of a mesh tree is the last two steps of a tree build over its fixed topology: boxes bottom-up (k_lbvh_boxes: leaf boxes =
// the triangle boxes, every internal node by the second child to arrive, child order per ordering by the rule of hk_bvh_rethread with
// ordering 0 kept as it is), then every node written at its place in every ordering (k_lbvh_emit)
void launch_mesh_tree_refit(hipStream_t st, const MeshTree& t, float4* lo, size_t ord_stride, uint32_t orderings) {
  LbvhBuffers b{};
  b.n = t.n;
  b.box_lo = t.tri_lo;
  b.box_hi = t.tri_hi;
  b.ids_sorted = t.leaf_shape;
  b.parent = t.parent; b.left = t.left; b.right = t.right; b.first = t.first; b.last = t.last;
  b.leaf_parent = t.leaf_parent;
  b.node_lo = t.node_lo;
  b.node_hi = t.node_hi;
  b.arrived = t.arrived;
  b.swap = t.swap;
  b.keep_order0 = 1u;
  if (t.n > 1u) (void)hipMemsetAsync(t.arrived, 0, (size_t)(t.n - 1u) * 4, st);
  const RefitScene none{};
  hipLaunchKernelGGL((k_lbvh_boxes<false>), dim3((t.n + 255u) / 256u), dim3(256), 0, st, none, b);
  const uint32_t threads = (2u * t.n - 1u) * orderings;
  hipLaunchKernelGGL(k_lbvh_emit, dim3((threads + 255u) / 256u), dim3(256), 0, st, b, lo, lo + 1, 2u, ord_stride, orderings);
}

// scratch of one tree build over n shapes: bytes, and the carving of a single allocation
size_t lbvh_scratch_bytes(uint32_t n, size_t* sort_temp_bytes) {
  size_t temp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 30);
  temp = (temp + 255) & ~(size_t)255;
  if (sort_temp_bytes) *sort_temp_bytes = temp;
  const size_t nn = ((size_t)n + 63) & ~(size_t)63;
  return 256 + temp + nn * (4 * 4 /* codes, ids x2 */ + 5 * 4 /* parent, left, right, first, last */ + 4 /* leaf_parent */ + 4 /* arrived */ + 4 /* swap (padded) */) +
         2 * nn * 2 * 16 /* node boxes, 2n - 1 */ + nn * (4 /* item_node[1] */ + 4 /* item_bucket, padded */ + 2 * 4 /* active lists */ + 54 * 4 + 4 * 4 + 14 * 4 + 2 * 4) /* SAH build */ +
         (nn / 1024 + 1) * 12 * 4 /* chunk_counts */;
}
// mode 0: LBVH (Morton order), mode 1: the reference's binned SAH (`bvh` 0.7.1).  `lo` / `hi` = the node array to overwrite,
// `stride` float4 between consecutive nodes (2: interleaved pairs, 1: two planes)
int launch_tree_build(hipStream_t st, int mode, bool light, const RefitScene& s, uint32_t n, const float4* box_lo, const float4* box_hi, void* scratch, float4* lo,
                      float4* hi, uint32_t stride, uint32_t orderings, size_t ord_stride, const MeshTree* keep, bool one_workgroup_top, bool mesh_tree, uint32_t* launches) {
  if (n == 0) return 0;
  mesh_tree = mesh_tree || keep;
  uint32_t launched = 2u;  // boxes, emit
  size_t temp = 0;
  (void)lbvh_scratch_bytes(n, &temp);
  const size_t nn = ((size_t)n + 63) & ~(size_t)63;
  uint8_t* p = (uint8_t*)scratch;
  LbvhBuffers b;
  b.n = n;
  b.box_lo = box_lo;
  b.box_hi = box_hi;
  b.keep_order0 = (mode == 1 || mesh_tree) ? 1u : 0u;  // (a mesh tree's ordering 0 is what its refit keeps: left before right)
  b.bounds = (float*)p; p += 256;
  void* sort_temp = p; p += temp;
  auto u32 = [&]() { uint32_t* q = (uint32_t*)p; p += nn * 4; return q; };
  b.codes = u32(); b.codes_sorted = u32(); b.ids = u32(); b.ids_sorted = u32();
  b.parent = u32(); b.left = u32(); b.right = u32(); b.first = u32(); b.last = u32(); b.leaf_parent = u32(); b.arrived = u32();
  b.swap = (uint8_t*)u32();
  b.node_lo = (float4*)p; p += 2 * nn * 16;
  b.node_hi = (float4*)p; p += 2 * nn * 16;
  (void)hipMemsetAsync(b.arrived, 0, nn * 4, st);
  (void)hipMemsetAsync(b.swap, 0, nn * 4, st);
  const dim3 per_shape((n + 255u) / 256u);
  if (mode == 1) {
    SahBuffers q;
    q.order[0] = b.codes; q.order[1] = b.codes_sorted;       // (the Morton arrays are free in this mode)
    q.item_node[0] = b.ids; q.item_node[1] = (uint32_t*)p; p += nn * 4;
    q.item_bucket = (uint8_t*)p; p += nn * 4;
    q.active[0] = (uint32_t*)p; p += nn * 4;
    q.active[1] = (uint32_t*)p; p += nn * 4;
    q.acc = (uint32_t*)p; p += nn * 54 * 4;
    q.split = (float*)p; p += nn * 4 * 4;
    q.offsets = (uint32_t*)p; p += nn * 14 * 4;
    q.node_level = (uint32_t*)p; p += nn * 4;
    q.roots = (uint32_t*)p; p += nn * 4;
    q.counters = (uint32_t*)b.bounds;                        // (256 B, unused by this mode)
    uint32_t* chunk_counts = (uint32_t*)p; p += (size_t)((n + 1023u) / 1024u) * 12 * 4;
    const dim3 subtrees((unsigned)std::min<size_t>(std::max<size_t>(n / 2, 1), 4096));
    launched += n > SAH_SUBTREE ? 2u : 1u;
    if (mesh_tree && n >= SAH_WIDE_MIN && !one_workgroup_top) {  // (mesh trees only: the instance tree and the light tree keep the one-workgroup top at any size)
      // the levels a balanced tree needs down to SAH_SUBTREE shapes per node, and six more for the lopsided splits of a real one
      uint32_t levels = 6u;
      while (((size_t)SAH_SUBTREE << (levels - 6u)) < n) ++levels;
      levels = std::min(levels, SAH_WIDE_MAX_LEVELS);
      const dim3 chunks((n + 1023u) / 1024u);
      launched += 1u + 5u * levels;
      hipLaunchKernelGGL(k_sahw_setup, chunks, dim3(1024), 0, st, b, q, levels);
      for (uint32_t level = 0; level < levels; ++level) {
        const dim3 per_node((unsigned)std::min<size_t>(((size_t)1 << std::min(level, 20u)) / 256 + 1, 256));  // (at most 2^level nodes)
        hipLaunchKernelGGL(k_sahw_bounds, chunks, dim3(1024), 0, st, b, q, level);
        hipLaunchKernelGGL(k_sahw_axis, per_node, dim3(256), 0, st, q, level);
        hipLaunchKernelGGL(k_sahw_buckets, chunks, dim3(1024), 0, st, b, q, level, chunk_counts);
        hipLaunchKernelGGL(k_sahw_split, per_node, dim3(256), 0, st, b, q, level, SAH_SUBTREE);
        hipLaunchKernelGGL(k_sahw_reorder, chunks, dim3(1024), 0, st, b, q, level, (const uint32_t*)chunk_counts);
      }
      hipLaunchKernelGGL(k_sahw_finish, per_shape, dim3(256), 0, st, b, q, levels);
      hipLaunchKernelGGL((k_sah_subtrees<false>), subtrees, dim3(1024), 0, st, s, b, q);
    } else if (light) {
      hipLaunchKernelGGL((k_sah_build<true>), dim3(1), dim3(1024), 0, st, s, b, q);
      if (n > SAH_SUBTREE) hipLaunchKernelGGL((k_sah_subtrees<true>), subtrees, dim3(1024), 0, st, s, b, q);
    } else {
      hipLaunchKernelGGL((k_sah_build<false>), dim3(1), dim3(1024), 0, st, s, b, q);
      if (n > SAH_SUBTREE) hipLaunchKernelGGL((k_sah_subtrees<false>), subtrees, dim3(1024), 0, st, s, b, q);
    }
  } else {
    if (light) {
      hipLaunchKernelGGL((k_lbvh_bounds<true>), dim3(1), dim3(1024), 0, st, s, b);
      hipLaunchKernelGGL((k_lbvh_codes<true>), per_shape, dim3(256), 0, st, s, b);
    } else {
      hipLaunchKernelGGL((k_lbvh_bounds<false>), dim3(1), dim3(1024), 0, st, s, b);
      hipLaunchKernelGGL((k_lbvh_codes<false>), per_shape, dim3(256), 0, st, s, b);
    }
    if (rocprim::radix_sort_pairs(sort_temp, temp, (const uint32_t*)b.codes, b.codes_sorted, (const uint32_t*)b.ids, b.ids_sorted, (size_t)n, 0, 30, st) != hipSuccess) return 1;
    if (n > 1) hipLaunchKernelGGL(k_lbvh_hierarchy, dim3((n + 254u) / 256u), dim3(256), 0, st, b);
    launched += 4u;  // (the sort counted as one)
  }
  if (launches) *launches += launched;
  if (light) hipLaunchKernelGGL((k_lbvh_boxes<true>), per_shape, dim3(256), 0, st, s, b);
  else hipLaunchKernelGGL((k_lbvh_boxes<false>), per_shape, dim3(256), 0, st, s, b);
  const uint32_t threads = (2u * n - 1u) * orderings;
  hipLaunchKernelGGL(k_lbvh_emit, dim3((threads + 255u) / 256u), dim3(256), 0, st, b, lo, hi, stride, ord_stride ? ord_stride : (size_t)(3u * n - 2u) * stride, orderings);
  if (keep) {  // the topology a later refit of this tree climbs (launch_mesh_tree_refit)
    const size_t ni = (size_t)(n - 1u) * 4;
    const std::pair<uint32_t*, const uint32_t*> planes[5] = {{keep->parent, b.parent}, {keep->left, b.left}, {keep->right, b.right}, {keep->first, b.first}, {keep->last, b.last}};
    for (const auto& pl : planes)
      if (ni) (void)hipMemcpyAsync(pl.first, pl.second, ni, hipMemcpyDeviceToDevice, st);
    if (ni) (void)hipMemcpyAsync(keep->leaf_parent, b.leaf_parent, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(keep->leaf_shape, b.ids_sorted, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// ---- a forest of mesh trees (hk_load_scene): scratch of one batch, and the build of every mesh of the batch into its own node range
static_assert(HK_FOREST_MESH_MAX_TRIANGLES + 1u == SAH_WIDE_MIN, "the forest takes every mesh below the multi-workgroup build");
static size_t forest_sort_temp(uint32_t n_tris, uint32_t n_meshes) {
  size_t temp = 0;
  (void)rocprim::segmented_radix_sort_pairs(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, n_tris, n_meshes,
                                            (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0, 30);
  return (temp + 255) & ~(size_t)255;
}
size_t forest_scratch_bytes(uint32_t n_tris, uint32_t n_meshes, int mode) {
  const size_t nn = ((size_t)n_tris + 63) & ~(size_t)63, mm = ((size_t)n_meshes + 63) & ~(size_t)63;
  size_t bytes = 256 + nn * (12 * 4) /* the arrays of launch_tree_build */ + 2 * nn * 2 * 16 /* node boxes */ + 2 * nn * 16 /* triangle boxes */ + nn * 4 /* item_mesh */ +
                 mm * (sizeof(ForestMesh) + 3 * 4 /* tops, segment offsets */ + 6 * 4 /* centre bounds */);
  if (mode == 1) bytes += nn * (4 + 4 + 2 * 4 + 54 * 4 + 4 * 4 + 14 * 4 + 2 * 4);
  else bytes += forest_sort_temp(n_tris, n_meshes);
  return bytes;
}
int launch_forest_build(hipStream_t st, int mode, const ForestMesh* meshes, uint32_t n_meshes, uint32_t n_tris, const float4* v0, const float4* v1, const float4* v2, void* scratch,
                        float4* nodes, uint32_t orderings, size_t ord_stride, uint32_t* launches) {
  if (n_meshes == 0 || n_tris == 0) return 0;
  const uint32_t n = n_tris;
  const size_t nn = ((size_t)n + 63) & ~(size_t)63, mm = ((size_t)n_meshes + 63) & ~(size_t)63;
  uint8_t* p = (uint8_t*)scratch;
  LbvhBuffers b;
  b.n = n;
  b.keep_order0 = 1u;  // (a mesh tree's ordering 0 is what its refit keeps: left before right)
  b.bounds = (float*)p; p += 256;
  auto u32 = [&](size_t count) { uint32_t* q = (uint32_t*)p; p += count * 4; return q; };
  b.codes = u32(nn); b.codes_sorted = u32(nn); b.ids = u32(nn); b.ids_sorted = u32(nn);
  b.parent = u32(nn); b.left = u32(nn); b.right = u32(nn); b.first = u32(nn); b.last = u32(nn); b.leaf_parent = u32(nn); b.arrived = u32(nn);
  b.swap = (uint8_t*)u32(nn);
  b.node_lo = (float4*)p; p += 2 * nn * 16;
  b.node_hi = (float4*)p; p += 2 * nn * 16;
  float4* tri_lo = (float4*)p; p += nn * 16;
  float4* tri_hi = (float4*)p; p += nn * 16;
  b.box_lo = tri_lo;
  b.box_hi = tri_hi;
  uint32_t* item_mesh = u32(nn);
  ForestMesh* d_meshes = (ForestMesh*)p; p += mm * sizeof(ForestMesh);
  uint32_t* d_tops = u32(mm);
  uint32_t* d_seg_begin = u32(mm);
  uint32_t* d_seg_end = u32(mm);
  float* d_mesh_bounds = (float*)u32(6 * mm);
  // (pageable sources: the copies have left the host buffers when the calls return)
  if (hipMemcpyAsync(d_meshes, meshes, (size_t)n_meshes * sizeof(ForestMesh), hipMemcpyHostToDevice, st) != hipSuccess) return 1;
  (void)hipMemsetAsync(b.arrived, 0, nn * 4, st);
  (void)hipMemsetAsync(b.swap, 0, nn * 4, st);
  (void)hipMemsetAsync(b.parent, (int)(FOREST_UNUSED & 0xFFu), nn * 4, st);
  (void)hipMemsetAsync(b.leaf_parent, 0xFF, nn * 4, st);
  (void)hipMemsetAsync(b.bounds, 0, 256, st);        // (the SAH build's counters)
  const RefitScene none{};
  const dim3 per_shape((n + 255u) / 256u);
  uint32_t launched = 0u;
  SahBuffers q{};
  if (mode == 1) {
    q.order[0] = b.codes; q.order[1] = b.codes_sorted;  // (the Morton arrays are free in this mode)
    q.item_node[0] = b.ids; q.item_node[1] = u32(nn);
    q.item_bucket = (uint8_t*)u32(nn);
    q.active[0] = u32(nn);
    q.active[1] = u32(nn);
    q.acc = u32(nn * 54);
    q.split = (float*)u32(nn * 4);
    q.offsets = u32(nn * 14);
    q.node_level = u32(nn);
    q.roots = u32(nn);
    q.counters = (uint32_t*)b.bounds;
    std::vector<uint32_t> tops;
    for (uint32_t m = 0; m < n_meshes; ++m)
      if (meshes[m].n_tris > SAH_SUBTREE) tops.push_back(m);
    if (!tops.empty() && hipMemcpyAsync(d_tops, tops.data(), tops.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_forest_setup, dim3(n_meshes), dim3(256), 0, st, (const ForestMesh*)d_meshes, n_meshes, v0, v1, v2, tri_lo, tri_hi, item_mesh, b, q, 1u);
    if (!tops.empty()) hipLaunchKernelGGL(k_forest_tops, dim3((unsigned)tops.size()), dim3(1024), 0, st, (const ForestMesh*)d_meshes, (const uint32_t*)d_tops, b, q);
    hipLaunchKernelGGL((k_sah_subtrees<false>), dim3((unsigned)std::min<size_t>(std::max<size_t>(n / 2, 1), 4096)), dim3(1024), 0, st, none, b, q);
    launched += tops.empty() ? 2u : 3u;
  } else {
    void* sort_temp = p;
    size_t temp = forest_sort_temp(n, n_meshes);
    std::vector<uint32_t> seg(2 * (size_t)n_meshes);
    for (uint32_t m = 0; m < n_meshes; ++m) {
      seg[m] = meshes[m].tri_begin;
      seg[n_meshes + m] = meshes[m].tri_begin + meshes[m].n_tris;
    }
    if (hipMemcpyAsync(d_seg_begin, seg.data(), (size_t)n_meshes * 4, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    if (hipMemcpyAsync(d_seg_end, seg.data() + n_meshes, (size_t)n_meshes * 4, hipMemcpyHostToDevice, st) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_forest_setup, dim3(n_meshes), dim3(256), 0, st, (const ForestMesh*)d_meshes, n_meshes, v0, v1, v2, tri_lo, tri_hi, item_mesh, b, q, 0u);
    hipLaunchKernelGGL(k_forest_lbvh_bounds, dim3(n_meshes), dim3(256), 0, st, (const ForestMesh*)d_meshes, b, d_mesh_bounds);
    hipLaunchKernelGGL(k_forest_lbvh_codes, per_shape, dim3(256), 0, st, (const uint32_t*)item_mesh, (const float*)d_mesh_bounds, b);
    if (rocprim::segmented_radix_sort_pairs(sort_temp, temp, (const uint32_t*)b.codes, b.codes_sorted, (const uint32_t*)b.ids, b.ids_sorted, n, n_meshes,
                                            (const uint32_t*)d_seg_begin, (const uint32_t*)d_seg_end, 0, 30, st) != hipSuccess)
      return 1;
    hipLaunchKernelGGL(k_forest_lbvh_hierarchy, per_shape, dim3(256), 0, st, (const ForestMesh*)d_meshes, (const uint32_t*)item_mesh, b);
    launched += 5u;  // (the sort counted as one)
  }
  hipLaunchKernelGGL((k_lbvh_boxes<false>), per_shape, dim3(256), 0, st, none, b);
  const uint32_t threads = (2u * n - 1u) * orderings;
  hipLaunchKernelGGL(k_forest_emit, dim3((threads + 255u) / 256u), dim3(256), 0, st, (const ForestMesh*)d_meshes, (const uint32_t*)item_mesh, b, nodes, ord_stride, orderings);
  launched += 2u;
  if (launches) *launches += launched;
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace hk
