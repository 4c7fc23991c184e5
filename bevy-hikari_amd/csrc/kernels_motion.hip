// kernels_motion.hip - motion vectors of deforming meshes (hikari_hip.h hk_set_mesh_motion_vectors; host side mesh_deform.hip; DESIGN 4
// "Motion vectors for deforming meshes"):
//   k_mesh_previous_fill  at enable time: the triangle planes of one mesh scattered into its per-vertex position plane
//   k_motion_velocity     behind every k_prepass while a mesh has live previous positions: velocity_uv.xy of the pixels whose closest hit
//                         lies on such a mesh, from the previous positions of the hit triangle's corners
// k_prepass itself is untouched (its instantiations, registers and scratch are pinned: tests/test_kernel_resources.py).  The pass finds
// the pixel's triangle again with the stackless one-mesh walk from global memory (hk_device.hpp traverse_bottom, ordering 0): no stack,
// no LDS copy of the scene, no scratch.  Background and static pixels leave after one 8-B load and one table look-up, a whole 8x8 tile
// of them per wave.
#include <hip/hip_runtime.h>

#include "hk_device.hpp"
#include "hk_kernels.hpp"
#include "hk_prepass.hpp"

namespace hkd {

// every corner writes its vertex (corners that share a vertex hold the same bits: whichever store lands last, the plane is the same);
// the w the deformation kernels write (kernels_deform.hip stage_vertex)
__global__ __launch_bounds__(256) void k_mesh_previous_fill(const float4* __restrict__ v0, const float4* __restrict__ v1, const float4* __restrict__ v2, uint32_t n_tris,
                                                            float4* __restrict__ pos, uint32_t n_vertices) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n_tris) return;
  const float4 q[3] = {v0[t], v1[t], v2[t]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t v = f2u(q[k].w);
    if (v < n_vertices) pos[v] = make_float4(q[k].x, q[k].y, q[k].z, 0.0f);
  }
}

__device__ __forceinline__ bool same_bits(const float4 a, const float4 b) { return f2u(a.x) == f2u(b.x) && f2u(a.y) == f2u(b.y) && f2u(a.z) == f2u(b.z); }

__global__ __launch_bounds__(256) void k_motion_velocity(DScene sc, DFrame fr, PrepassParams pp, GBuffer g, MotionTable mt, int row_begin, int row_end) {
  const Pixel px = pixel_of_thread<false>(fr.dw, row_begin, row_end);
  bool rewritten = false;
  if (px.valid) {
    const int idx = px.x + fr.dw * px.y;
    const float2 im = g.instance_material[idx];
    const uint32_t instance = im.x > 0.0f ? f32_to_u32(im.x) : HK_U32_MAX;  // (the miss branch stores 0, an instance its id + 0.5)
    MotionEntry entry{nullptr, 0u, 0u};
    if (instance < mt.n_instances) entry = mt.entries[instance];
    const float4* __restrict__ prev = entry.previous;
    if (prev) {
      const DInstance& in = sc.instances[instance];
      // the pixel's primary ray, the bits k_prepass formed, into the instance's local space as traverse_top does at an instance entry
      const Ray ray = primary_ray(fr, pp, (float)px.x, (float)px.y);
      Ray lr;
      lr.origin = world_to_local_position(in, ray.origin);
      lr.direction = world_to_local_direction(in, ray.direction);
      lr.inv_direction = 1.0f / lr.direction;
      RayCounters rc{0, 0};
      // The walk is a chain of dependent fetches from global memory, and the longest one of the launch is the launch's time.  The prepass
      // stored the hit's world position = origin + direction * distance with |direction| = 1, so the distance is known to a few ulp:
      // a walk that starts with a bound a little beyond it (1e-4 relative) skips every subtree whose box the ray enters behind the hit
      // and finds the same closest triangle with the same arithmetic.  (After a second trip of the prepass the position is measured
      // from the near point, which lies on the ray: the bound from the eye holds all the same.)
      const float4 position_depth = g.position[idx];
      const f3 world_position = F3(position_depth.x, position_depth.y, position_depth.z);
      Hit hit;
      hit.uv = F2(0.0f, 0.0f);
      hit.distance = length(world_position - ray.origin) * 1.0001f + 1e-6f;
      hit.instance_index = instance;
      hit.primitive_index = HK_U32_MAX;
      bool found = traverse_bottom(sc, hit, lr, in.node_offset, in.node_count, in.primitive, 0.0f, rc);
      if (found && !fr.is_ortho) {  // clip_at_near_plane: a hit in front of the near plane - the prepass traced once more from the plane itself
        const f3 near_point = primary_near_point(fr, pp, (float)px.x, (float)px.y);
        if (hit.distance < length(near_point - ray.origin)) {
          lr.origin = world_to_local_position(in, near_point);
          hit.uv = F2(0.0f, 0.0f);
          hit.distance = HK_F32_MAX;
          hit.primitive_index = HK_U32_MAX;
          found = traverse_bottom(sc, hit, lr, in.node_offset, in.node_count, in.primitive, 0.0f, rc);
        }
      }
      // (a miss: an exact tie the two walks broke differently - the stored velocity stays)
      if (found) {
        const float4 q0 = sc.tri_v0[hit.primitive_index], q1 = sc.tri_v1[hit.primitive_index], q2 = sc.tri_v2[hit.primitive_index];
        const uint32_t i0 = f2u(q0.w), i1 = f2u(q1.w), i2 = f2u(q2.w);
        if (i0 < entry.n_vertices && i1 < entry.n_vertices && i2 < entry.n_vertices) {
          const float4 P0 = prev[i0], P1 = prev[i1], P2 = prev[i2];  // three independent 16-B gathers, in flight together
          // previous corners equal to the current ones bit for bit: the pixel keeps what the prepass wrote
          if (!(same_bits(P0, q0) && same_bits(P1, q1) && same_bits(P2, q2))) {
            const f2 b = hit.uv;
            const f3 prev_local = xyz(P0) + b.x * (xyz(P1) - xyz(P0)) + b.y * (xyz(P2) - xyz(P0));
            f4 previous_world;
            if (in.moved) {
              const float4* pm = pp.prev_models + 4u * instance;
              previous_world = mul(pm[0], pm[1], pm[2], pm[3], F4(prev_local, 1.0f));
            } else {
              previous_world = mul(in.m0, in.m1, in.m2, in.m3, F4(prev_local, 1.0f));
            }
            const f4 clip = mul(pp.vp0, pp.vp1, pp.vp2, pp.vp3, F4(world_position, 1.0f));  // (world_position exactly as the prepass formed it)
            const f2 velocity = clip_to_uv(clip) - clip_to_uv(mul(pp.pvp0, pp.pvp1, pp.pvp2, pp.pvp3, previous_world));
            *reinterpret_cast<float2*>(g.velocity_uv + idx) = make_float2(velocity.x, velocity.y);  // (.zw, the mesh uv, stays)
            rewritten = true;
          }
        }
      }
    }
  }
  if (mt.rewritten) {  // (the debug count: one atomic per wave that rewrote anything)
    const unsigned long long m = __ballot(rewritten);
    if (m != 0ull && wave_leader()) atomicAdd(mt.rewritten, (unsigned int)__popcll(m));
  }
}

}  // namespace hkd

namespace hk {
using namespace hkd;

void launch_mesh_previous_fill(hipStream_t st, const float4* v0, const float4* v1, const float4* v2, uint32_t n_tris, float4* pos, uint32_t n_vertices) {
  if (!n_tris) return;
  hipLaunchKernelGGL(k_mesh_previous_fill, dim3((n_tris + 255u) / 256u), dim3(256), 0, st, v0, v1, v2, n_tris, pos, n_vertices);
}

void launch_motion_velocity(hipStream_t st, const DScene& sc, const DFrame& fr, const float* inverse_view_proj, const float* view_proj, const float* prev_view_proj,
                            const float4* prev_models, float jitter_x, float jitter_y, const GBuffer& g, const MotionTable& mt, int y0, int y1) {
  if (y1 <= y0) return;
  const PrepassParams pp = make_prepass_params(inverse_view_proj, view_proj, prev_view_proj, prev_models, jitter_x, jitter_y, nullptr);
  hipLaunchKernelGGL(k_motion_velocity, grid_for(fr.dw, y1 - y0), dim3(256), 0, st, sc, fr, pp, g, mt, y0, y1);
}

}  // namespace hk
