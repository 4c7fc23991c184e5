// kernels_deform.hip - new vertex data of one mesh, or of many in one call, on the device (hk_update_mesh_vertices, hk_skin_mesh,
// hk_deform_meshes, hk_deform_meshes_device; host side mesh_deform.hip):
// the vertices of the mesh land in its normal plane and in a position scratch plane, the mesh box is reduced on the way, then every
// triangle of the mesh takes its three positions into the triangle planes and its box into the refit's leaf boxes (kernels_tree.hip
// launch_mesh_tree_refit carries on from there).  Streaming kernels, one thread per vertex / per triangle.
#include <hip/hip_runtime.h>

#include "hk_box.hpp"
#include "hk_device.hpp"
#include "hk_kernels.hpp"

namespace hkd {

namespace {
// the mesh box as six order-preserving words (hk_box.hpp box_word; decoded by kernels_scene.hip k_mesh_instances): atomicMin / atomicMax
// give the min / max over the vertices whatever order they arrive in.  One wave reduces its lanes' positions, lane 0 adds them to the six words (words 0-2 min, 3-5 max)
__device__ __forceinline__ void reduce_box(uint32_t* box, bool valid, float x, float y, float z) {
  uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  if (valid) {
    const float p[3] = {x, y, z};
    for (int k = 0; k < 3; ++k) mn[k] = mx[k] = box_word(p[k]);
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 3; ++k) {
      mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], off));
      mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], off));
    }
  // (an atomic that would change nothing is not issued: the six words only ever shrink / grow during a launch, so whatever value of
  // this launch the load sees, a wave that does not beat it cannot beat the current one.  Without the test every wave of a large mesh
  // queues on the same six addresses, and the launch takes the time of those atomics, not of its memory traffic.)
  if ((threadIdx.x & 63u) == 0u && mx[0] != 0u)
    for (int k = 0; k < 3; ++k) {
      if (mn[k] < __hip_atomic_load(&box[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&box[k], mn[k]);
      if (mx[k] > __hip_atomic_load(&box[3 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&box[3 + k], mx[k]);
    }
}

// one vertex of hk_update_mesh_vertices: positions / normals (3 floats per vertex, pinned host memory, read once; hk_deform_meshes_device:
// the caller's device memory, `ps` / `ns` floats from one vertex to the next)
__device__ __forceinline__ void stage_vertex(const float* __restrict__ positions, const float* __restrict__ normals, uint32_t v, float4* __restrict__ pos,
                                             float4* __restrict__ vn, float& x, float& y, float& z, uint32_t ps = 3u, uint32_t ns = 3u) {
  const float* p = positions + (size_t)ps * v;
  x = p[0];
  y = p[1];
  z = p[2];
  pos[v] = make_float4(x, y, z, 0.0f);
  if (normals) {
    const float* q = normals + (size_t)ns * v;
    vn[v] = make_float4(q[0], q[1], q[2], 0.0f);
  }
}

// Linear-blend skinning of one vertex, Bevy 0.9 skinning.wgsl (hikari_hip.h hk_skin_mesh; DESIGN "Mesh deformation"): fixed order, no contraction.
//   M  = ((w.x J[i.x] + w.y J[i.y]) + w.z J[i.z]) + w.w J[i.w]               element by element
//   p' = ((M0 x + M1 y) + M2 z) + M3                                           (M0..M3: columns)
//   n' = ((c0 n.x + c1 n.y) + c2 n.z),  (c0, c1, c2) = (M1 x M2, M2 x M0, M0 x M1) / dot(M2, M0 x M1)   (inverse_transpose_3x3)
// n' is stored as it comes out (hit_info normalises, as for any uploaded normal).
// `p` / `q`: the vertex's bind position and normal (HK_DEFORM_SKIN: of the skin's bind planes; HK_DEFORM_MORPH_SKIN: morphed, in registers)
__device__ __forceinline__ void skin_vertex(const float4 p, const float4 q, const uint2* __restrict__ joints, const float4* __restrict__ weights,
                                            const float4* __restrict__ joint_mats, uint32_t v, float4* __restrict__ pos, float4* __restrict__ vn, float& px,
                                            float& py, float& pz) {
  const uint2 jw = joints[v];
  const uint32_t j[4] = {jw.x & 0xFFFFu, jw.x >> 16, jw.y & 0xFFFFu, jw.y >> 16};
  const float4 w4 = weights[v];
  const float w[4] = {w4.x, w4.y, w4.z, w4.w};
  float m[4][4];  // m[column][row]
  for (int c = 0; c < 4; ++c) {
    const float4 a = joint_mats[4u * j[0] + c];
    m[c][0] = w[0] * a.x;
    m[c][1] = w[0] * a.y;
    m[c][2] = w[0] * a.z;
    m[c][3] = w[0] * a.w;
  }
  for (int t = 1; t < 4; ++t)
    for (int c = 0; c < 4; ++c) {
      const float4 a = joint_mats[4u * j[t] + c];
      m[c][0] = m[c][0] + w[t] * a.x;
      m[c][1] = m[c][1] + w[t] * a.y;
      m[c][2] = m[c][2] + w[t] * a.z;
      m[c][3] = m[c][3] + w[t] * a.w;
    }
  px = ((m[0][0] * p.x + m[1][0] * p.y) + m[2][0] * p.z) + m[3][0];
  py = ((m[0][1] * p.x + m[1][1] * p.y) + m[2][1] * p.z) + m[3][1];
  pz = ((m[0][2] * p.x + m[1][2] * p.y) + m[2][2] * p.z) + m[3][2];
  pos[v] = make_float4(px, py, pz, 0.0f);
  auto cross = [](const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  const float* c0 = m[0];
  const float* c1 = m[1];
  const float* c2 = m[2];
  float x[3], y[3], z[3];
  cross(c1, c2, x);
  cross(c2, c0, y);
  cross(c0, c1, z);
  const float det = (c2[0] * z[0] + c2[1] * z[1]) + c2[2] * z[2];
  for (int k = 0; k < 3; ++k) {
    x[k] = x[k] / det;
    y[k] = y[k] / det;
    z[k] = z[k] / det;
  }
  vn[v] = make_float4((x[0] * q.x + y[0] * q.y) + z[0] * q.z, (x[1] * q.x + y[1] * q.y) + z[1] * q.z, (x[2] * q.x + y[2] * q.y) + z[2] * q.z, 0.0f);
}

// Morph targets of one vertex (hikari_hip.h hk_set_mesh_morph_targets; DESIGN "Mesh deformation"): fixed order, no contraction.
//   p = ((base + w[a1] dp[a1]) + w[a2] dp[a2]) + ...   per component over the ACTIVE targets a1 < a2 < ... (k_deform_begin's list),
// normals alike with dn (NORMALS) or the base normals as they are.  The list, its length and the weights are the same for every vertex
// of the item: scalar loads.  The deltas are packed planes of 3 floats per vertex, one per target: the 64 vertices of a wave read 768
// consecutive bytes of a plane.  Four targets' loads are issued before the first is used; the additions stay in list order.
// (The pointers of an item come out of the staged table, so the compiler knows nothing of where they point: the casts below tell it
// that the list and the weights are constant memory - written by the launch before - and the planes global memory, which makes the
// former scalar loads and the latter global loads.)
template <typename T>
using uniform_ptr = const T __attribute__((address_space(4)))*;
template <typename T>
using global_ptr = const T __attribute__((address_space(1)))*;
template <bool NORMALS>
__device__ __forceinline__ void morph_vertex(const DeformItem* __restrict__ it, uint32_t v, float p[3], float q[3]) {
  const auto bp = (global_ptr<float>)(uintptr_t)(it->morph_base_p + 3 * (size_t)v);
  const auto bn = (global_ptr<float>)(uintptr_t)(it->morph_base_n + 3 * (size_t)v);
  for (int c = 0; c < 3; ++c) {
    p[c] = bp[c];
    q[c] = bn[c];
  }
  const auto active = (uniform_ptr<uint32_t>)(uintptr_t)it->morph_active;
  const auto w = (uniform_ptr<float>)(uintptr_t)it->morph_w;
  const size_t plane = 3 * (size_t)it->n_vertices;
  const auto dp = (global_ptr<float>)(uintptr_t)it->morph_dp + 3 * (size_t)v;
  const auto dn = (global_ptr<float>)(uintptr_t)it->morph_dn + (NORMALS ? 3 * (size_t)v : 0);
  const uint32_t n = active[it->n_targets];
  uint32_t i = 0;
  for (; i + 4u <= n; i += 4u) {
    float wk[4], d[4][3], e[4][3];
    for (int t = 0; t < 4; ++t) {
      const uint32_t k = active[i + t];
      wk[t] = w[k];
      const auto a = dp + plane * k;
      for (int c = 0; c < 3; ++c) d[t][c] = a[c];
      if (NORMALS) {
        const auto b = dn + plane * k;
        for (int c = 0; c < 3; ++c) e[t][c] = b[c];
      }
    }
    for (int t = 0; t < 4; ++t)
      for (int c = 0; c < 3; ++c) {
        p[c] = p[c] + wk[t] * d[t][c];
        if (NORMALS) q[c] = q[c] + wk[t] * e[t][c];
      }
  }
  for (; i < n; ++i) {
    const uint32_t k = active[i];
    const float wk = w[k];
    const auto a = dp + plane * k;
    for (int c = 0; c < 3; ++c) p[c] = p[c] + wk * a[c];
    if (NORMALS) {
      const auto b = dn + plane * k;
      for (int c = 0; c < 3; ++c) q[c] = q[c] + wk * b[c];
    }
  }
}

// triangle t of the mesh: its three positions (the w words - vertex indices - stay) and its box (light.wgsl:408-412, the leaf box)
// `face` (or NULL): the triangle's un-normalised face vector e1 x e2, e1 = p1 - p0, e2 = p2 - p0 (hikari_hip.h HK_DEFORM_RECOMPUTE_NORMALS)
__device__ __forceinline__ void mesh_triangle(const float4* __restrict__ pos, float4* __restrict__ v0, float4* __restrict__ v1, float4* __restrict__ v2, uint32_t t,
                                              float4* __restrict__ tri_lo, float4* __restrict__ tri_hi, float4* __restrict__ face = nullptr) {
  float4 q[3] = {v0[t], v1[t], v2[t]};
  for (int k = 0; k < 3; ++k) {
    const float4 p = pos[f2u(q[k].w)];
    q[k] = make_float4(p.x, p.y, p.z, q[k].w);
  }
  v0[t] = q[0];
  v1[t] = q[1];
  v2[t] = q[2];
  triangle_box(q[0], q[1], q[2], tri_lo[t], tri_hi[t]);
  if (face) {
    const float ax = q[1].x - q[0].x, ay = q[1].y - q[0].y, az = q[1].z - q[0].z;
    const float bx = q[2].x - q[0].x, by = q[2].y - q[0].y, bz = q[2].z - q[0].z;
    face[t] = make_float4(ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx, 0.0f);
  }
}
}  // namespace

__global__ __launch_bounds__(256) void k_mesh_stage(const float* __restrict__ positions, const float* __restrict__ normals, uint32_t n, float4* __restrict__ pos,
                                                    float4* __restrict__ vn, uint32_t* __restrict__ box) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  const bool valid = v < n;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  if (valid) stage_vertex(positions, normals, v, pos, vn, x, y, z);
  reduce_box(box, valid, x, y, z);
}

__global__ __launch_bounds__(256) void k_mesh_skin(const float4* __restrict__ bind_pos, const float4* __restrict__ bind_nrm, const uint2* __restrict__ joints,
                                                   const float4* __restrict__ weights, const float4* __restrict__ joint_mats, uint32_t n, float4* __restrict__ pos,
                                                   float4* __restrict__ vn, uint32_t* __restrict__ box) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  const bool valid = v < n;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (valid) skin_vertex(bind_pos[v], bind_nrm[v], joints, weights, joint_mats, v, pos, vn, px, py, pz);
  reduce_box(box, valid, px, py, pz);
}

__global__ __launch_bounds__(256) void k_mesh_triangles(const float4* __restrict__ pos, float4* __restrict__ v0, float4* __restrict__ v1, float4* __restrict__ v2,
                                                        uint32_t n_tris, float4* __restrict__ tri_lo, float4* __restrict__ tri_hi) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n_tris) return;
  mesh_triangle(pos, v0, v1, v2, t, tri_lo, tri_hi);
}

// ------------------------------------------------------------------ many meshes in one call (hk_deform_meshes)
// The same three steps over ALL items of a batch: the launches do not depend on how many there are.  Every workgroup works on 256
// consecutive vertices / triangles of ONE item (hk_kernels.hpp SegmentBlock, a table the host writes), so the wave-wide box reduction
// never mixes two meshes and an item may have any size.  The item records and the tables are read from the call's pinned staging block.
// One workgroup per item: its box words back to the empty box (min words all ones, max words zero), and - a skin item - its joint
// matrices into device memory, where the vertex kernel reads each of them once per vertex; a morph item's weights likewise, with the
// list of the active targets the vertex kernel loops over.
__global__ __launch_bounds__(256) void k_deform_begin(const DeformItem* __restrict__ items, uint32_t n_items) {
  if (blockIdx.x >= n_items) return;
  const DeformItem* it = items + blockIdx.x;
  uint32_t* box = it->box;
  if (threadIdx.x < 6u) box[threadIdx.x] = threadIdx.x < 3u ? 0xFFFFFFFFu : 0u;
  const uint32_t kind = it->kind;
  if (kind == HK_DEFORM_SKIN || kind == HK_DEFORM_MORPH_SKIN) {
    const float4* __restrict__ src = it->palette;
    float4* __restrict__ dst = it->joint_mats;
    const uint32_t n = 4u * it->n_joints;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) dst[i] = src[i];
  }
  if (kind != HK_DEFORM_MORPH && kind != HK_DEFORM_MORPH_SKIN) return;
  // a morph item: its weights into the mesh's own copy, and the ascending list of the targets whose weight does not compare equal to
  // zero (NaN: active).  256 targets per round: a ballot per wave, the lanes below in the ballot, the waves below through LDS - the
  // place of a target in the list depends on the weights alone.
  __shared__ uint32_t wave_count[4];
  const float* __restrict__ src = it->morph_src;
  float* __restrict__ dst = it->morph_w;
  uint32_t* __restrict__ active = it->morph_active;
  const uint32_t n = it->n_targets, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t total = 0;
  for (uint32_t first = 0; first < n; first += 256u) {
    const uint32_t k = first + threadIdx.x;
    bool on = false;
    if (k < n) {
      const float w = src[k];
      dst[k] = w;
      on = w != 0.0f;
    }
    const unsigned long long mask = __ballot(on);
    if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t at = total + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t q = 0; q < 4u; ++q) {
      if (q < wave) at += wave_count[q];
      total += wave_count[q];
    }
    if (on) active[at] = k;
    __syncthreads();
  }
  if (threadIdx.x == 0u) active[n] = total;
}
// (five workgroups per CU, as before the morph branch: without the bound the skin's matrix loads are hoisted over the morph loop and cost a wave)
__global__ __launch_bounds__(256, 5) void k_deform_vertices(const DeformItem* __restrict__ items, const SegmentBlock* __restrict__ blocks) {
  const SegmentBlock bl = blocks[blockIdx.x];
  const DeformItem* it = items + bl.segment;
  const uint32_t v = bl.first + threadIdx.x;
  const bool valid = v < it->n_vertices;
  float4* pos = it->pos;
  float4* vn = it->vn;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  const uint32_t kind = it->kind;
  if (kind == HK_DEFORM_VERTICES) {
    if (valid) stage_vertex(it->positions, it->normals, v, pos, vn, x, y, z, it->pos_stride, it->nrm_stride);
  } else if (valid) {
    // the bind pose of the skin, or the morphed vertex: stored as it is (MORPH) or skinned in its place (MORPH_SKIN)
    float4 p, q;
    if (kind == HK_DEFORM_SKIN) {
      p = it->bind_pos[v];
      q = it->bind_nrm[v];
    } else {
      float a[3], b[3];
      if (it->morph_dn) morph_vertex<true>(it, v, a, b);
      else morph_vertex<false>(it, v, a, b);
      p = make_float4(a[0], a[1], a[2], 0.0f);
      q = make_float4(b[0], b[1], b[2], 0.0f);
    }
    if (kind == HK_DEFORM_MORPH) {
      x = p.x;
      y = p.y;
      z = p.z;
      pos[v] = p;
      vn[v] = q;
    } else {
      skin_vertex(p, q, it->joints, it->weights, it->joint_mats, v, pos, vn, x, y, z);
    }
  }
  reduce_box(it->box, valid, x, y, z);
}
// ... and the arrival counters of the item's tree (one per internal node = per triangle but the last) back to zero for the climb
__global__ __launch_bounds__(256) void k_deform_triangles(const DeformItem* __restrict__ items, const SegmentBlock* __restrict__ blocks) {
  const SegmentBlock bl = blocks[blockIdx.x];
  const DeformItem* it = items + bl.segment;
  const uint32_t t = bl.first + threadIdx.x, n = it->n_tris;
  if (t >= n) return;
  if (t + 1u < n) it->tree.arrived[t] = 0u;
  mesh_triangle(it->pos, it->v0, it->v1, it->v2, t, it->tree.tri_lo, it->tree.tri_hi, it->face);
}
// HK_DEFORM_RECOMPUTE_NORMALS: vertex v's normal = ((+0 + f[t_1]) + f[t_2]) + ... over its corner list, in list order - a gather, so the
// result is the same whatever the scheduling.  An all-zero sum (no triangle names v, or areas that cancel) keeps the normal there is.
// `blocks` holds the vertex workgroups of the flagged items only.
__global__ __launch_bounds__(256) void k_deform_normals(const DeformItem* __restrict__ items, const SegmentBlock* __restrict__ blocks) {
  const SegmentBlock bl = blocks[blockIdx.x];
  const DeformItem* it = items + bl.segment;
  const uint32_t v = bl.first + threadIdx.x;
  if (v >= it->n_vertices) return;
  const uint32_t* __restrict__ tri = it->corner_tri;
  const float4* __restrict__ face = it->face;
  const uint32_t b = it->corner_off[v], e = it->corner_off[v + 1u];
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (uint32_t i = b; i < e; ++i) {
    const float4 f = face[tri[i]];
    sx = sx + f.x;
    sy = sy + f.y;
    sz = sz + f.z;
  }
  if (sx == 0.0f && sy == 0.0f && sz == 0.0f) return;
  it->vn[v] = make_float4(sx, sy, sz, 0.0f);
}

// ... the boxes alone, of triangles nobody has moved yet (hk_rebuild_mesh_tree on a mesh never deformed)
__global__ __launch_bounds__(256) void k_mesh_triangle_boxes(const float4* __restrict__ v0, const float4* __restrict__ v1, const float4* __restrict__ v2, uint32_t n_tris,
                                                             float4* __restrict__ tri_lo, float4* __restrict__ tri_hi) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n_tris) return;
  triangle_box(v0[t], v1[t], v2[t], tri_lo[t], tri_hi[t]);
}

}  // namespace hkd

namespace hk {
using namespace hkd;

void launch_mesh_stage(hipStream_t st, const float* positions, const float* normals, uint32_t n, float4* pos, float4* vn, uint32_t* box) {
  if (n) hipLaunchKernelGGL(k_mesh_stage, dim3((n + 255u) / 256u), dim3(256), 0, st, positions, normals, n, pos, vn, box);
}
void launch_mesh_skin(hipStream_t st, const float4* bind_pos, const float4* bind_nrm, const uint2* joints, const float4* weights, const float4* joint_mats, uint32_t n,
                      float4* pos, float4* vn, uint32_t* box) {
  if (n) hipLaunchKernelGGL(k_mesh_skin, dim3((n + 255u) / 256u), dim3(256), 0, st, bind_pos, bind_nrm, joints, weights, joint_mats, n, pos, vn, box);
}
void launch_mesh_triangles(hipStream_t st, const float4* pos, float4* v0, float4* v1, float4* v2, uint32_t n_tris, float4* tri_lo, float4* tri_hi) {
  if (n_tris) hipLaunchKernelGGL(k_mesh_triangles, dim3((n_tris + 255u) / 256u), dim3(256), 0, st, pos, v0, v1, v2, n_tris, tri_lo, tri_hi);
}
void launch_mesh_triangle_boxes(hipStream_t st, const float4* v0, const float4* v1, const float4* v2, uint32_t n_tris, float4* tri_lo, float4* tri_hi) {
  if (n_tris) hipLaunchKernelGGL(k_mesh_triangle_boxes, dim3((n_tris + 255u) / 256u), dim3(256), 0, st, v0, v1, v2, n_tris, tri_lo, tri_hi);
}
void launch_deform_batch(hipStream_t st, const DeformItem* items, uint32_t n_items, const SegmentBlock* vertex_blocks, uint32_t n_vertex_blocks,
                         const SegmentBlock* triangle_blocks, uint32_t n_triangle_blocks, const SegmentBlock* node_blocks, uint32_t n_node_blocks, size_t ord_stride,
                         uint32_t orderings, hipEvent_t sources_read, const SegmentBlock* normal_blocks, uint32_t n_normal_blocks) {
  if (!n_items) return;
  hipLaunchKernelGGL(k_deform_begin, dim3(n_items), dim3(256), 0, st, items, n_items);
  hipLaunchKernelGGL(k_deform_vertices, dim3(n_vertex_blocks), dim3(256), 0, st, items, vertex_blocks);
  if (sources_read) (void)hipEventRecord(sources_read, st);
  hipLaunchKernelGGL(k_deform_triangles, dim3(n_triangle_blocks), dim3(256), 0, st, items, triangle_blocks);
  if (n_normal_blocks) hipLaunchKernelGGL(k_deform_normals, dim3(n_normal_blocks), dim3(256), 0, st, items, normal_blocks);
  launch_deform_tree_refit(st, items, triangle_blocks, n_triangle_blocks, node_blocks, n_node_blocks, ord_stride, orderings);
}

}  // namespace hk
