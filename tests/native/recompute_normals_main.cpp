// A stand-alone host program over scene_builder.cpp / host_logic.cpp alone (no HIP runtime), meant to be built with
// -fsanitize=address,undefined (tests/test_deform_device.py does so): hk_scene_builder_recompute_mesh_normals on a bent grid, a mesh with
// a vertex no triangle names and a zero-area triangle, an unknown id, and the finishes around them.  Exit status 0 and "ok" on success.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hikari_hip.h"

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #cond, hk_last_error()); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

int main() {
  hk_scene_builder* b = nullptr;
  CHECK(hk_scene_builder_create(&b) == HK_OK);
  // a 17 x 17 grid, bent out of its plane
  const int side = 17;
  std::vector<float> pos, nrm, uv;
  std::vector<uint32_t> idx;
  for (int j = 0; j < side; ++j)
    for (int i = 0; i < side; ++i) {
      const float x = (float)i / (side - 1) - 0.5f, z = (float)j / (side - 1) - 0.5f;
      pos.insert(pos.end(), {x, 0.0f, z});
      nrm.insert(nrm.end(), {0.0f, 1.0f, 0.0f});
      uv.insert(uv.end(), {x + 0.5f, z + 0.5f});
    }
  for (int j = 0; j + 1 < side; ++j)
    for (int i = 0; i + 1 < side; ++i) {
      const uint32_t a = j * side + i, c = (j + 1) * side + i;
      idx.insert(idx.end(), {a, c, a + 1, a + 1, c, c + 1});
    }
  uint32_t grid = 0, odd = 0, material = 0, instance = 0;
  CHECK(hk_scene_builder_add_mesh(b, pos.data(), nrm.data(), uv.data(), (uint32_t)pos.size() / 3, idx.data(), (uint32_t)idx.size(), HK_TOPOLOGY_TRIANGLE_LIST, &grid) == HK_OK);
  // two triangles and a collinear one over six vertices: vertex 2 is named by nobody, vertex 5 by the zero-area triangle alone
  const float opos[18] = {0, 0, 0, 1, 0, 0, 9, 9, 9, 0, 0, 1, 1, 0, 1, 2, 0, 0};
  const float onrm[18] = {0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1};
  const float ouv[12] = {0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0};
  const uint32_t oidx[9] = {0, 3, 1, 1, 3, 4, 0, 1, 5};
  CHECK(hk_scene_builder_add_mesh(b, opos, onrm, ouv, 6, oidx, 9, HK_TOPOLOGY_TRIANGLE_LIST, &odd) == HK_OK);
  HkMaterial m;
  memset(&m, 0, sizeof(m));
  m.base_color[0] = m.base_color[1] = m.base_color[2] = m.base_color[3] = 0.8f;
  m.base_color_texture = m.emissive_texture = m.metallic_roughness_texture = m.normal_map_texture = m.occlusion_texture = HK_NO_TEXTURE;
  CHECK(hk_scene_builder_add_material(b, &m, &material) == HK_OK);
  const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  CHECK(hk_scene_builder_add_instance(b, grid, material, identity, &instance) == HK_OK);
  CHECK(hk_scene_builder_add_instance(b, odd, material, identity, &instance) == HK_OK);
  CHECK(hk_scene_builder_finish(b) == HK_OK);

  for (size_t v = 0; v < pos.size() / 3; ++v) pos[3 * v + 1] = 0.2f * sinf(5.0f * pos[3 * v]) * cosf(4.0f * pos[3 * v + 2]);
  CHECK(hk_scene_builder_set_mesh_vertices(b, grid, pos.data(), nullptr) == HK_OK);
  CHECK(hk_scene_builder_recompute_mesh_normals(b, grid) == HK_OK);
  CHECK(hk_scene_builder_recompute_mesh_normals(b, odd) == HK_OK);
  CHECK(hk_scene_builder_recompute_mesh_normals(b, 2) == HK_E_INVALID);
  CHECK(hk_scene_builder_recompute_mesh_normals(nullptr, 0) == HK_E_INVALID);
  CHECK(hk_scene_builder_finish(b) == HK_OK);

  const HkVertex* vertices = nullptr;
  uint32_t n = 0;
  HkMeshIndex gi, oi;
  CHECK(hk_scene_builder_vertices(b, &vertices, &n) == HK_OK);
  CHECK(hk_scene_builder_mesh_index(b, grid, &gi) == HK_OK && hk_scene_builder_mesh_index(b, odd, &oi) == HK_OK);
  CHECK(gi.vertex + (uint32_t)pos.size() / 3 <= n && oi.vertex + 6 <= n);
  for (uint32_t v = 0; v < (uint32_t)pos.size() / 3; ++v) {
    const float* q = vertices[gi.vertex + v].normal;
    CHECK(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && q[1] > 0.0f);
  }
  CHECK(memcmp(vertices[oi.vertex + 2].normal, onrm + 6, 12) == 0);   // named by nobody: kept
  CHECK(memcmp(vertices[oi.vertex + 5].normal, onrm + 15, 12) == 0);  // named by the zero-area triangle alone: kept
  CHECK(vertices[oi.vertex + 0].normal[1] == 1.0f && vertices[oi.vertex + 4].normal[1] == 1.0f);
  hk_scene_builder_destroy(b);
  printf("ok\n");
  return 0;
}
