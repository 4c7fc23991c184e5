// kernels_query.hip - ray queries of a host against the device scene (hikari_hip.h hk_cast_rays / hk_cast_rays_device):
//   k_cast_rays   one ray per lane: closest hit (the reference's traverse_top with early_distance = 0) or occlusion (first hit)
// The rays are a host's: arbitrary origins, an arbitrary count, no tile of neighbouring pixels and no frame behind them.  The walks
// are the frame's own (hk_device.hpp traverse_top / traverse_flat, hk_wide.hpp traverse_top_wide) on the frame's own staging
// (hk_light.hpp stage_scene), so a query meets the same candidates in the same order as a primary ray of the same context; there
// is no arithmetic here that those kernels do not have.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hk_device.hpp"
#include "hk_kernels.hpp"
#include "hk_light.hpp"
#include "hk_wide.hpp"

namespace hkd {

// A ray that is not walked (hikari_hip.h): a component of origin / direction that is not finite, a direction of all zeros, a
// max_distance that is NaN or negative.  Decided on the bits and by comparisons, before any walk.
__device__ __forceinline__ bool query_not_finite(float v) { return (f2u(v) & 0x7F800000u) == 0x7F800000u; }
__device__ __forceinline__ bool query_ray_invalid(const float4& a, const float4& b) {
  const bool not_finite = query_not_finite(a.x) || query_not_finite(a.y) || query_not_finite(a.z) || query_not_finite(b.x) || query_not_finite(b.y) || query_not_finite(b.z);
  const bool no_direction = b.x == 0.0f && b.y == 0.0f && b.z == 0.0f;
  return not_finite || no_direction || !(a.w >= 0.0f);
}

// MODE: hk_light.hpp stage_scene (0 global memory, the skip-link walk in the ray's ordering; 1 LDS copy, two-level walk; 2 LDS copy,
// one-level walk; 4 global memory, the wide walk - closest hits only).
// rays: two float4 per ray (origin, max_distance | direction, exclude_instance bits); hits: three float4 per ray (distance, instance,
// primitive, material | barycentric, uv | normal, status) - HkRay / HkRayHit.
// A lane takes rays i, i + lanes, i + 2 lanes ...: modes 0 - 2 are launched with a lane per ray; the wide walk with at most as many
// lanes as the trace stages' own launch (kernels_wavefront.hip wide_trace_lanes), because the entries of a lane's stack beyond its 28
// in LDS live in the context's spill area, which is sized for that launch (hk_wide.hpp WideStackSpill) - no private array, no scratch.
template <int MODE, bool ANY, bool ATTRIBUTES>
__global__ __launch_bounds__(256) void k_cast_rays(DScene gsc, WideTrees wide, const float4* __restrict__ rays, uint32_t n, float4* __restrict__ hits) {
  const DScene sc = stage_scene<MODE>(gsc);  // (every thread of the workgroup copies: the tail guard comes after the barrier inside)
  __shared__ uint32_t wide_lds[MODE == 4 ? HK_WIDE_LDS_STACK * 256u : 1u];
  const size_t lanes = (size_t)gridDim.x * 256u, lane = (size_t)blockIdx.x * 256u + threadIdx.x;
#pragma unroll 1
  for (size_t i = lane; i < n; i += lanes) {
    const float4 a = rays[2u * i], b = rays[2u * i + 1u];
    Hit hit;
    hit.uv = F2(0.0f, 0.0f);
    hit.distance = a.w;
    hit.instance_index = HK_U32_MAX;
    hit.primitive_index = HK_U32_MAX;
    Ray ray;
    ray.origin = F3(a.x, a.y, a.z);
    ray.direction = F3(b.x, b.y, b.z);
    ray.inv_direction = 1.0f / ray.direction;
    const bool invalid = query_ray_invalid(a, b);
    if (!invalid) {
      const uint32_t exclude = f2u(b.w);
      const float early = ANY ? __builtin_inff() : 0.0f;  // light.wgsl:421-423: a hit nearer than early_distance ends the walk
      RayCounters rc{0, 0};
      if (MODE == 4) {
        WideStackSpill stack{wide_lds, wide.spill, lanes, lane, wide.lost};
        hit = traverse_top_wide<false>(sc, wide, ray, a.w, early, exclude, stack, rc);
      } else {
        hit = traverse_top(sc, ray, a.w, early, exclude, rc);
      }
    }
    const bool found = hit.instance_index != HK_U32_MAX;
    uint32_t material = 0u;
    f2 uv = F2(0.0f, 0.0f);
    f3 normal = F3(0.0f, 0.0f, 0.0f);
    if (ATTRIBUTES && !invalid) {
      const HitInfo info = hit_info(sc, ray, hit);
      material = info.material_index;
      uv = info.uv;
      normal = info.normal;
    }
    const uint32_t status = invalid ? HK_RAY_INVALID : (found ? HK_RAY_HIT : HK_RAY_MISS);
    float4* __restrict__ out = hits + 3u * i;
    out[0] = make_float4(hit.distance, u2f(hit.instance_index), u2f(hit.primitive_index), u2f(material));
    out[1] = make_float4(hit.uv.x, hit.uv.y, uv.x, uv.y);
    out[2] = make_float4(normal.x, normal.y, normal.z, u2f(status));
  }
}

}  // namespace hkd

namespace hk {
using namespace hkd;

// Which walk answers: the one the frame's own closest-hit rays take on this scene (kernels.hip launch_prepass) - the LDS copy where
// the scene fits it (one-level where DScene::flat_mode holds), otherwise global memory: the wide walk for closest hits when the
// caller hands its records (`wide` with tlas and spill != nullptr; wide_lanes = the lanes the spill area serves), the skip-link walk in
// the ray's ordering for everything else.
void launch_cast_rays(hipStream_t st, const DScene& sc, const WideTrees* wide, size_t wide_lanes, const void* rays, uint32_t n, uint32_t flags, void* hits) {
  if (!n) return;
  const dim3 grid((unsigned)(((size_t)n + 255u) / 256u));
  const size_t lds = (size_t)sc.blob_f4 * 16 <= HK_LDS_SCENE_BYTES ? (size_t)sc.blob_f4 * 16 : 0;
  const bool flat = sc.flat_mode != 0u && lds;
  const bool any = (flags & HK_RAYS_ANY) != 0u, attributes = (flags & HK_RAYS_ATTRIBUTES) != 0u;
  const bool use_wide = !lds && !any && wide && wide->tlas && wide->spill && wide_lanes >= 256u;
  const dim3 wide_grid((unsigned)std::min<size_t>(grid.x, wide_lanes / 256u));
  const WideTrees wt = use_wide ? *wide : WideTrees{};
  const float4* r = (const float4*)rays;
  float4* h = (float4*)hits;
#define HK_LAUNCH(M, L) \
  do {                                                                                                                    \
    if (any) hipLaunchKernelGGL((k_cast_rays<M, true, false>), grid, dim3(256), L, st, sc, wt, r, n, h);                   \
    else if (attributes) hipLaunchKernelGGL((k_cast_rays<M, false, true>), grid, dim3(256), L, st, sc, wt, r, n, h);       \
    else hipLaunchKernelGGL((k_cast_rays<M, false, false>), grid, dim3(256), L, st, sc, wt, r, n, h);                      \
  } while (0)
  if (flat) HK_LAUNCH(2, lds);
  else if (lds) HK_LAUNCH(1, lds);
  else if (use_wide && attributes) hipLaunchKernelGGL((k_cast_rays<4, false, true>), wide_grid, dim3(256), 0, st, sc, wt, r, n, h);
  else if (use_wide) hipLaunchKernelGGL((k_cast_rays<4, false, false>), wide_grid, dim3(256), 0, st, sc, wt, r, n, h);
  else HK_LAUNCH(0, 0);
#undef HK_LAUNCH
}

}  // namespace hk
