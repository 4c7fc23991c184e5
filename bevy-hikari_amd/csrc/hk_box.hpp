// hk_box.hpp - the box arithmetic of the scene kernels (kernels_scene.hip, kernels_tree.hip, kernels_deform.hip), defined once: every
// box the device derives must be the host builder's bit for bit, so the order of the operands and the treatment of zeros are part of it.
#pragma once
#include "hk_device.hpp"

namespace hkd {

// std::min / std::max of the host builder (scene_builder.cpp): the first operand on a tie, whatever the signs of zeros
HKD float hmin(float a, float b) { return b < a ? b : a; }
HKD float hmax(float a, float b) { return a < b ? b : a; }
// the host's leaf boxes (hk_context.hpp hmin / hmax, build_static_region): IEEE minNum / maxNum with -0 < +0
HKD float leaf_min(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? a : b;
  return a < b ? a : b;
}
HKD float leaf_max(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? b : a;
  return a > b ? a : b;
}
// a float as a u32 whose unsigned order is the float order with -0 < +0 (atomicMin / atomicMax over floats in any order), and back
HKD uint32_t box_word(float f) {
  const uint32_t u = f2u(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
HKD float box_unword(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// the box of one triangle (light.wgsl:408-412, the leaf box); the w words are zero
HKD void triangle_box(const float4 a, const float4 b, const float4 c, float4& lo, float4& hi) {
  lo = make_float4(leaf_min(a.x, leaf_min(b.x, c.x)), leaf_min(a.y, leaf_min(b.y, c.y)), leaf_min(a.z, leaf_min(b.z, c.z)), 0.0f);
  hi = make_float4(leaf_max(a.x, leaf_max(b.x, c.x)), leaf_max(a.y, leaf_max(b.y, c.y)), leaf_max(a.z, leaf_max(b.z, c.z)), 0.0f);
}

}  // namespace hkd
