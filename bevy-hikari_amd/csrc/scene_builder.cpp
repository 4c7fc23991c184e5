// scene_builder.cpp - host-side Prepare-stage work of the path, re-implemented in C++.
//
// Mirrors (reference paths relative to cryscan/bevy-hikari v0.3.15):
//   mesh -> primitives + BLAS      src/mesh_material/mod.rs:379-467  (TryFrom<Mesh> for GpuMesh)
//   flat skip-link node format     src/mesh_material/mod.rs:177-201  (GpuNode::pack) on top of
//                                  the `bvh` crate =0.7.1 (Cargo.toml:21): BVH::build is a
//                                  recursive 6-bucket SAH split on the largest centroid axis,
//                                  flatten_custom a depth-first [navigator L, subtree L,
//                                  navigator R, subtree R] emission with EMPTY leaf boxes.  The
//                                  crate is not vendored in the reference checkout; the algorithm
//                                  is restated from its published source.
//   global buffers + offsets       src/mesh_material/mesh.rs:106-166
//   instance AABB / TLAS / emissive list / alias tables / light BVH
//                                  src/mesh_material/instance.rs:286-428, mod.rs:306-376
//
// Pure host code: no HIP calls, usable without a GPU.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "hk_internal.hpp"

namespace hk {

namespace {

struct Box {
  float mn[3], mx[3];
  static Box empty() {
    const float inf = std::numeric_limits<float>::infinity();
    return Box{{inf, inf, inf}, {-inf, -inf, -inf}};
  }
  void grow(const float p[3]) {
    for (int k = 0; k < 3; ++k) {
      mn[k] = std::min(mn[k], p[k]);
      mx[k] = std::max(mx[k], p[k]);
    }
  }
  void join(const Box& o) {
    for (int k = 0; k < 3; ++k) {
      mn[k] = std::min(mn[k], o.mn[k]);
      mx[k] = std::max(mx[k], o.mx[k]);
    }
  }
  float size(int k) const { return mx[k] - mn[k]; }
  float center(int k) const { return mn[k] + size(k) / 2.0f; }
  float surface_area() const {
    float x = size(0), y = size(1), z = size(2);
    return 2.0f * (x * y + x * z + y * z);
  }
  int largest_axis() const {
    float x = size(0), y = size(1), z = size(2);
    if (x > y && x > z) return 0;
    if (y > z) return 1;
    return 2;
  }
};

// ---- `bvh` 0.7.1: BVHNode::build
struct TreeNode {
  bool leaf;
  uint32_t shape;       // leaf
  Box child_l, child_r; // inner
  int l, r;             // inner: indices into the tree vector
};

int build_recursive(const std::vector<Box>& shapes, const std::vector<uint32_t>& indices, std::vector<TreeNode>& nodes) {
  Box bounds = Box::empty(), centroids = Box::empty();
  for (uint32_t i : indices) {
    bounds.join(shapes[i]);
    float c[3] = {shapes[i].center(0), shapes[i].center(1), shapes[i].center(2)};
    centroids.grow(c);
  }
  if (indices.size() == 1) {
    nodes.push_back(TreeNode{true, indices[0], Box::empty(), Box::empty(), -1, -1});
    return (int)nodes.size() - 1;
  }
  const int node_index = (int)nodes.size();
  nodes.push_back(TreeNode{false, 0, Box::empty(), Box::empty(), -1, -1});

  const int axis = centroids.largest_axis();
  const float axis_size = centroids.mx[axis] - centroids.mn[axis];
  std::vector<uint32_t> left, right;
  Box lbox = Box::empty(), rbox = Box::empty();
  if (axis_size < 0.00001f) {
    // shapes too close together: split the index list in half
    size_t half = indices.size() / 2;
    left.assign(indices.begin(), indices.begin() + half);
    right.assign(indices.begin() + half, indices.end());
    for (uint32_t i : left) lbox.join(shapes[i]);
    for (uint32_t i : right) rbox.join(shapes[i]);
  } else {
    const int NUM_BUCKETS = 6;
    Box bucket_box[NUM_BUCKETS];
    uint32_t bucket_size[NUM_BUCKETS];
    std::vector<uint32_t> assign[NUM_BUCKETS];
    for (int b = 0; b < NUM_BUCKETS; ++b) {
      bucket_box[b] = Box::empty();
      bucket_size[b] = 0;
    }
    for (uint32_t i : indices) {
      float rel = (shapes[i].center(axis) - centroids.mn[axis]) / axis_size;
      int b = (int)(rel * ((float)NUM_BUCKETS - 0.01f));
      b = std::min(std::max(b, 0), NUM_BUCKETS - 1);
      bucket_box[b].join(shapes[i]);
      bucket_size[b] += 1;
      assign[b].push_back(i);
    }
    int min_bucket = 0;
    float min_cost = std::numeric_limits<float>::infinity();
    for (int i = 0; i < NUM_BUCKETS - 1; ++i) {
      Box l = Box::empty(), r = Box::empty();
      uint32_t ln = 0, rn = 0;
      for (int b = 0; b <= i; ++b) { l.join(bucket_box[b]); ln += bucket_size[b]; }
      for (int b = i + 1; b < NUM_BUCKETS; ++b) { r.join(bucket_box[b]); rn += bucket_size[b]; }
      float cost = ((float)ln * l.surface_area() + (float)rn * r.surface_area()) / bounds.surface_area();
      if (cost < min_cost) {
        min_bucket = i;
        min_cost = cost;
        lbox = l;
        rbox = r;
      }
    }
    for (int b = 0; b <= min_bucket; ++b) left.insert(left.end(), assign[b].begin(), assign[b].end());
    for (int b = min_bucket + 1; b < NUM_BUCKETS; ++b) right.insert(right.end(), assign[b].begin(), assign[b].end());
    if (left.empty() || right.empty()) {  // degenerate SAH (NaN costs): fall back to the half split
      left.clear(); right.clear();
      size_t half = indices.size() / 2;
      left.assign(indices.begin(), indices.begin() + half);
      right.assign(indices.begin() + half, indices.end());
      lbox = Box::empty(); rbox = Box::empty();
      for (uint32_t i : left) lbox.join(shapes[i]);
      for (uint32_t i : right) rbox.join(shapes[i]);
    }
  }
  int l = build_recursive(shapes, left, nodes);
  int r = build_recursive(shapes, right, nodes);
  nodes[node_index].child_l = lbox;
  nodes[node_index].child_r = rbox;
  nodes[node_index].l = l;
  nodes[node_index].r = r;
  return node_index;
}

// GpuNode::pack, mod.rs:185-201
HkNode pack_node(const Box& box, uint32_t entry_index, uint32_t exit_index, uint32_t shape_index) {
  HkNode n;
  if (entry_index == 0xFFFFFFFFu) entry_index = shape_index | HK_BVH_LEAF_FLAG;
  for (int k = 0; k < 3; ++k) {
    n.min[k] = box.mn[k];
    n.max[k] = box.mx[k];
  }
  n.entry_index = entry_index;
  n.exit_index = exit_index;
  return n;
}

// `bvh` 0.7.1: BVHNode::flatten_custom / create_flat_branch
uint32_t flatten(const std::vector<TreeNode>& nodes, int idx, std::vector<HkNode>& out, uint32_t next_free);
uint32_t flat_branch(const std::vector<TreeNode>& nodes, const Box& box, int child, std::vector<HkNode>& out, uint32_t next_free) {
  out.push_back(pack_node(Box::empty(), 0, 0, 0));  // dummy, replaced below
  uint32_t after = flatten(nodes, child, out, next_free + 1);
  out[next_free] = pack_node(box, next_free + 1, after, 0xFFFFFFFFu);
  return after;
}
uint32_t flatten(const std::vector<TreeNode>& nodes, int idx, std::vector<HkNode>& out, uint32_t next_free) {
  const TreeNode& n = nodes[idx];
  if (n.leaf) {
    out.push_back(pack_node(Box::empty(), 0xFFFFFFFFu, next_free + 1, n.shape));
    return next_free + 1;
  }
  uint32_t nf = flat_branch(nodes, n.child_l, n.l, out, next_free);
  nf = flat_branch(nodes, n.child_r, n.r, out, nf);
  return nf;
}

}  // namespace

std::vector<HkNode> build_flat_bvh(const std::vector<float>& boxes_min_max /* n x 6 */) {
  const size_t n = boxes_min_max.size() / 6;
  std::vector<HkNode> out;
  if (n == 0) return out;
  std::vector<Box> shapes(n);
  std::vector<uint32_t> indices(n);
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) {
      shapes[i].mn[k] = boxes_min_max[6 * i + k];
      shapes[i].mx[k] = boxes_min_max[6 * i + 3 + k];
    }
    indices[i] = (uint32_t)i;
  }
  std::vector<TreeNode> tree;
  tree.reserve(2 * n);
  build_recursive(shapes, indices, tree);
  out.reserve(3 * n);
  flatten(tree, 0, out, 0);
  return out;
}

// A VALID flat tree over the same shapes without the SAH work: the index list halved recursively, O(n log n) box unions.  It is
// what hk_scene_builder_finish_instances uploads when the device is about to build the real trees (hk_update_scene_instances):
// the right size, every leaf present, correct navigator boxes - a frame rendered from it would still be right, only slower.
static int build_halving(const std::vector<Box>& shapes, uint32_t begin, uint32_t end, std::vector<TreeNode>& nodes, Box* box_out) {
  if (end - begin == 1) {
    nodes.push_back(TreeNode{true, begin, Box::empty(), Box::empty(), -1, -1});
    *box_out = shapes[begin];
    return (int)nodes.size() - 1;
  }
  const int node_index = (int)nodes.size();
  nodes.push_back(TreeNode{false, 0, Box::empty(), Box::empty(), -1, -1});
  const uint32_t mid = begin + (end - begin) / 2;
  Box lb, rb;
  const int l = build_halving(shapes, begin, mid, nodes, &lb);
  const int r = build_halving(shapes, mid, end, nodes, &rb);
  nodes[node_index].child_l = lb;
  nodes[node_index].child_r = rb;
  nodes[node_index].l = l;
  nodes[node_index].r = r;
  *box_out = lb;
  box_out->join(rb);
  return node_index;
}
std::vector<HkNode> build_flat_placeholder(const std::vector<float>& boxes_min_max /* n x 6 */) {
  const size_t n = boxes_min_max.size() / 6;
  std::vector<HkNode> out;
  if (n == 0) return out;
  std::vector<Box> shapes(n);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      shapes[i].mn[k] = boxes_min_max[6 * i + k];
      shapes[i].mx[k] = boxes_min_max[6 * i + 3 + k];
    }
  std::vector<TreeNode> tree;
  tree.reserve(2 * n);
  Box all;
  build_halving(shapes, 0u, (uint32_t)n, tree, &all);
  out.reserve(3 * n);
  flatten(tree, 0, out, 0);
  return out;
}

// ------------------------------------------------------------------------------------------
struct BuilderMesh {
  std::vector<HkVertex> vertices;
  std::vector<HkPrimitive> primitives;
  std::vector<HkNode> nodes;
  float aabb_center[3], aabb_half[3];
  bool pending = false;  // added by hk_scene_builder_add_mesh_deferred: `nodes` is a valid stand-in of the final size until the tree is built
  // declared by hk_scene_builder_declare_mesh and not filled yet: vertices and primitives are zeros of the final counts (and `pending` is set);
  // the declaration's index count (0: the identity list) and topology, which whoever fills the mesh assembles by
  bool unresolved = false;
  uint32_t decl_indices = 0, decl_topology = 0;
};
struct BuilderInstance {
  uint32_t mesh, material;
  float transform[16];
};

}  // namespace hk

struct hk_scene_builder {
  std::vector<hk::BuilderMesh> meshes;
  std::vector<HkMaterial> materials;
  std::vector<hk::BuilderInstance> instance_decl;
  bool finished = false;
  bool standin_trees = false;             // finished by hk_scene_builder_finish_instances: the two trees are valid stand-ins, not the reference's
  bool meshes_dirty = true;               // the concatenated mesh buffers must be brought up to date
  size_t concat_meshes = 0;               // ... from this mesh on: the earlier ones are in them as they stand (meshes added after a finish are appended)
  std::vector<float> finished_transforms;  // transforms at the last finish ...
  std::vector<float> previous_transforms;  // ... and at the one before (PreviousMeshUniform)
  // outputs
  std::vector<HkVertex> vertices;
  std::vector<HkPrimitive> primitives;
  std::vector<HkNode> asset_nodes;
  std::vector<HkMeshIndex> mesh_index;
  std::vector<HkMeshExtent> last_extent;   // per mesh the last finish saw, its ranges in THAT finish's arrays (hk_scene_builder_remove_mesh erases with the mesh)
  std::vector<HkInstance> instances;
  std::vector<HkNode> instance_nodes;
  std::vector<HkEmissive> emissives;
  std::vector<HkNode> emissive_nodes;
  std::vector<HkAliasEntry> alias_table;
};

namespace hk {
namespace {

void mat_point(const float m[16], const float p[3], float out[3]) {  // glam Mat4::transform_point3
  for (int k = 0; k < 3; ++k) out[k] = m[k] * p[0] + m[4 + k] * p[1] + m[8 + k] * p[2] + m[12 + k];
}
void mat_vector(const float m[16], const float p[3], float out[3]) {  // glam Mat4::transform_vector3
  for (int k = 0; k < 3; ++k) out[k] = m[k] * p[0] + m[4 + k] * p[1] + m[8 + k] * p[2];
}
// inverse().transpose() of an (arbitrary) 4x4, evaluated in double and rounded once
bool inverse_transpose(const float m[16], float out[16]) {
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
  double det = a[0] * inv[0] + a[1] * inv[4] + a[2] * inv[8] + a[3] * inv[12];
  if (det == 0.0) return false;
  double id = 1.0 / det;
  // out = transpose(inverse): out[col*4+row] = inv[row*4+col]
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) out[c * 4 + r] = (float)(inv[r * 4 + c] * id);
  return true;
}

// GpuMesh::transformed_primitive_areas, mod.rs:307-318
std::vector<float> primitive_areas(const BuilderMesh& mesh, const float transform[16]) {
  std::vector<float> areas;
  areas.reserve(mesh.primitives.size());
  for (const HkPrimitive& p : mesh.primitives) {
    float v[3][3];
    for (int k = 0; k < 3; ++k) mat_point(transform, mesh.vertices[p.vertices[k].index].position, v[k]);
    float a[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
    float b[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
    float c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    areas.push_back(0.5f * fabsf(sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])));
  }
  return areas;
}

// GpuMesh::build_alias_table, mod.rs:320-376
std::vector<HkAliasEntry> build_alias_table(const std::vector<float>& areas) {
  const size_t n = areas.size();
  std::vector<HkAliasEntry> table;
  if (n == 0) return table;
  float surface_area = 0.0f;
  for (float a : areas) surface_area += a;
  const float mean_area = surface_area / (float)n;
  struct Bucket { size_t id; float prob; };
  std::vector<Bucket> over, under;
  for (size_t i = 0; i < n; ++i) {
    float p = areas[i] / mean_area;
    if (p > 1.0f) over.push_back({i, p});
  }
  for (size_t i = 0; i < n; ++i) {
    float p = areas[i] / mean_area;
    if (p < 1.0f) under.push_back({i, p});
  }
  table.resize(n);
  for (size_t i = 0; i < n; ++i) table[i] = HkAliasEntry{0.0f, (uint32_t)i};
  while (!under.empty() && !over.empty()) {
    Bucket over_bucket = over.back();
    over.pop_back();
    Bucket under_bucket = under.back();
    under.pop_back();
    float delta = 1.0f - under_bucket.prob;
    over_bucket.prob -= delta;
    if (over_bucket.prob > 1.0f)
      over.push_back(over_bucket);
    else if (over_bucket.prob < 1.0f)
      under.push_back(over_bucket);
    table[under_bucket.id] = HkAliasEntry{delta, (uint32_t)over_bucket.id};
  }
  return table;
}

}  // namespace
}  // namespace hk

namespace hk {
bool instance_world_record(const float transform[16], const float aabb_center[3], const float aabb_half[3], float mn_out[3], float mx_out[3], float itm[16]) {
  float center[3];
  mat_point(transform, aabb_center, center);
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};  // seeded at zero, instance.rs:298-299
  for (int corner = 0; corner < 8; ++corner) {
    float e[3] = {aabb_half[0] * (float)(2 * (corner & 1) - 1), aabb_half[1] * (float)(2 * ((corner >> 1) & 1) - 1), aabb_half[2] * (float)(2 * ((corner >> 2) & 1) - 1)};
    float t[3];
    mat_vector(transform, e, t);
    for (int k = 0; k < 3; ++k) {
      mn[k] = std::min(mn[k], t[k]);
      mx[k] = std::max(mx[k], t[k]);
    }
  }
  for (int k = 0; k < 3; ++k) {
    mn_out[k] = mn[k] + center[k];
    mx_out[k] = mx[k] + center[k];
  }
  return inverse_transpose(transform, itm);
}
bool builder_has_standin_trees(const hk_scene_builder* b) { return b && b->finished && b->standin_trees; }
uint32_t builder_instance_count(const hk_scene_builder* b) { return b ? (uint32_t)b->instance_decl.size() : 0u; }
bool builder_instance_decl(const hk_scene_builder* b, uint32_t i, InstanceDecl* out) {
  // (poses set since the last finish are exactly what the caller is after; the MESH buffers must be the finished ones)
  if (!b || b->meshes_dirty || b->mesh_index.size() != b->meshes.size() || i >= b->instance_decl.size()) return false;
  const BuilderInstance& d = b->instance_decl[i];
  out->mesh = b->mesh_index[d.mesh];
  out->material = d.material;
  out->transform = d.transform;
  out->aabb_center = b->meshes[d.mesh].aabb_center;
  out->aabb_half = b->meshes[d.mesh].aabb_half;
  return true;
}
// which instances emit (instance.rs:380-382): the intensity of a material's emissive colour, 255 a |rgb|; an instance is an emitter iff it is > 0
float emissive_intensity(const float e[4]) { return 255.0f * e[3] * sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]); }
bool material_emits(const HkMaterial& m) { return emissive_intensity(m.emissive) > 0.0f; }
void builder_materials(const hk_scene_builder* b, const HkMaterial** p, uint32_t* n) {
  *p = b->materials.data();
  *n = (uint32_t)b->materials.size();
}
void builder_commit_transforms(hk_scene_builder* b) {
  std::vector<float> now(b->instance_decl.size() * 16);
  for (size_t i = 0; i < b->instance_decl.size(); ++i) memcpy(&now[16 * i], b->instance_decl[i].transform, 64);
  b->previous_transforms = now;
  const size_t common = std::min(now.size(), b->finished_transforms.size());
  if (common) memcpy(b->previous_transforms.data(), b->finished_transforms.data(), common * sizeof(float));
  b->finished_transforms.swap(now);
}
}  // namespace hk

using namespace hk;

extern "C" {

int hk_scene_builder_create(hk_scene_builder** out) {
  HK_REQUIRE(out, HK_E_INVALID, "out is NULL");
  *out = new (std::nothrow) hk_scene_builder();
  HK_REQUIRE(*out, HK_E_NOMEM, "allocation failed");
  return HK_OK;
}
void hk_scene_builder_destroy(hk_scene_builder* b) { delete b; }

static int add_mesh_impl(hk_scene_builder* b, const float* positions, const float* normals, const float* uvs, uint32_t n_vertices, const uint32_t* indices,
                         uint32_t n_indices, uint32_t topology, uint32_t* mesh_id, bool deferred) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  // mod.rs:383-397: position, normal and uv0 are all required
  HK_REQUIRE(positions && normals && uvs && n_vertices > 0, HK_E_INVALID, "mesh needs position, normal and uv attributes");
  HK_REQUIRE(topology == HK_TOPOLOGY_TRIANGLE_LIST || topology == HK_TOPOLOGY_TRIANGLE_STRIP, HK_E_UNSUPPORTED, "incompatible primitive topology");
  BuilderMesh mesh;
  mesh.vertices.resize(n_vertices);
  float mn[3] = {positions[0], positions[1], positions[2]}, mx[3] = {positions[0], positions[1], positions[2]};
  for (uint32_t i = 0; i < n_vertices; ++i) {
    HkVertex& v = mesh.vertices[i];
    for (int k = 0; k < 3; ++k) {
      v.position[k] = positions[3 * i + k];
      v.normal[k] = normals[3 * i + k];
      mn[k] = std::min(mn[k], v.position[k]);
      mx[k] = std::max(mx[k], v.position[k]);
    }
    v.u = uvs[2 * i];
    v.v = uvs[2 * i + 1];
  }
  for (int k = 0; k < 3; ++k) {  // bevy Aabb::from_min_max
    mesh.aabb_center[k] = 0.5f * (mx[k] + mn[k]);
    mesh.aabb_half[k] = 0.5f * (mx[k] - mn[k]);
  }
  std::vector<uint32_t> idx;
  if (indices && n_indices) {
    idx.assign(indices, indices + n_indices);
  } else {  // mod.rs:408-411
    idx.resize(n_vertices);
    for (uint32_t i = 0; i < n_vertices; ++i) idx[i] = i;
  }
  for (uint32_t i : idx) HK_REQUIRE(i < n_vertices, HK_E_INVALID, "vertex index out of range");
  auto push = [&](uint32_t a, uint32_t c, uint32_t d) {
    HkPrimitive p;
    uint32_t id[3] = {a, c, d};
    for (int k = 0; k < 3; ++k) {
      memcpy(p.vertices[k].position, mesh.vertices[id[k]].position, 12);
      p.vertices[k].index = id[k];
    }
    mesh.primitives.push_back(p);
  };
  if (topology == HK_TOPOLOGY_TRIANGLE_LIST) {  // mod.rs:414-431
    HK_REQUIRE(idx.size() % 3 == 0, HK_E_UNSUPPORTED, "incompatible primitive topology (index count not a multiple of 3)");
    for (size_t i = 0; i + 2 < idx.size(); i += 3) push(idx[i], idx[i + 1], idx[i + 2]);
  } else {  // mod.rs:432-449: odd triangles flip winding
    for (size_t i = 0; i + 2 < idx.size(); ++i) {
      if ((i & 1) == 0)
        push(idx[i], idx[i + 1], idx[i + 2]);
      else
        push(idx[i + 1], idx[i], idx[i + 2]);
    }
  }
  HK_REQUIRE(!mesh.primitives.empty(), HK_E_INVALID, "mesh has no primitive");  // mod.rs:454-456
  std::vector<float> boxes;
  boxes.reserve(mesh.primitives.size() * 6);
  for (const HkPrimitive& p : mesh.primitives) {
    Box bx = Box::empty();
    for (int k = 0; k < 3; ++k) bx.grow(p.vertices[k].position);
    boxes.insert(boxes.end(), bx.mn, bx.mn + 3);
    boxes.insert(boxes.end(), bx.mx, bx.mx + 3);
  }
  // mod.rs:458-459; a deferred mesh gets a valid stand-in of the final size (any binary tree over n shapes has 3n - 2 nodes)
  mesh.nodes = deferred ? build_flat_placeholder(boxes) : build_flat_bvh(boxes);
  mesh.pending = deferred;
  b->meshes.push_back(std::move(mesh));
  b->meshes_dirty = true;
  b->finished = false;
  if (mesh_id) *mesh_id = (uint32_t)b->meshes.size() - 1;
  return HK_OK;
}

int hk_scene_builder_add_mesh(hk_scene_builder* b, const float* positions, const float* normals, const float* uvs, uint32_t n_vertices,
                              const uint32_t* indices, uint32_t n_indices, uint32_t topology, uint32_t* mesh_id) {
  return add_mesh_impl(b, positions, normals, uvs, n_vertices, indices, n_indices, topology, mesh_id, false);
}
int hk_scene_builder_add_mesh_deferred(hk_scene_builder* b, const float* positions, const float* normals, const float* uvs, uint32_t n_vertices,
                                       const uint32_t* indices, uint32_t n_indices, uint32_t topology, uint32_t* mesh_id) {
  return add_mesh_impl(b, positions, normals, uvs, n_vertices, indices, n_indices, topology, mesh_id, true);
}
int hk_scene_builder_pending_mesh_trees(const hk_scene_builder* b, uint32_t* count) {
  HK_REQUIRE(b && count, HK_E_INVALID, "NULL argument");
  *count = builder_pending_mesh_count(b);
  return HK_OK;
}


// A mesh known by its counts alone (hikari_hip.h): zeros of the final sizes and the deferred mesh's stand-in, so that every offset and
// HkMeshIndex record is final at the next finish; hk_add_meshes_device or hk_scene_builder_resolve_mesh fills it.
static uint32_t declared_triangles(uint32_t n_vertices, uint32_t n_indices, uint32_t topology) {
  const uint32_t n = n_indices ? n_indices : n_vertices;  // mod.rs:408-411
  if (topology == HK_TOPOLOGY_TRIANGLE_LIST) return n / 3u;
  return n >= 3u ? n - 2u : 0u;
}
// build_flat_placeholder over n shapes that are all the point 0, emitted directly: the halved index list in the flatten_custom layout
// (every box is the zero box then, so no tree is kept and no union is formed - a declaration costs its node array alone)
static uint32_t emit_zero_standin(uint32_t begin, uint32_t end, std::vector<HkNode>& out, uint32_t next_free) {
  HkNode n{};
  if (end - begin == 1u) {  // pack_node(Box::empty(), leaf)
    const float inf = std::numeric_limits<float>::infinity();
    for (int k = 0; k < 3; ++k) { n.min[k] = inf; n.max[k] = -inf; }
    n.entry_index = begin | HK_BVH_LEAF_FLAG;
    n.exit_index = next_free + 1u;
    out.push_back(n);
    return next_free + 1u;
  }
  const uint32_t mid = begin + (end - begin) / 2u;
  const uint32_t halves[3] = {begin, mid, end};
  for (int h = 0; h < 2; ++h) {  // create_flat_branch: the navigator, then the subtree it skips
    const uint32_t at = next_free;
    out.push_back(n);
    next_free = emit_zero_standin(halves[h], halves[h + 1], out, at + 1u);
    out[at].entry_index = at + 1u;
    out[at].exit_index = next_free;
  }
  return next_free;
}
int hk_scene_builder_declare_mesh(hk_scene_builder* b, uint32_t n_vertices, uint32_t n_indices, uint32_t topology, uint32_t* mesh_id) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_REQUIRE(n_vertices > 0, HK_E_INVALID, "mesh needs position, normal and uv attributes");
  HK_REQUIRE(topology == HK_TOPOLOGY_TRIANGLE_LIST || topology == HK_TOPOLOGY_TRIANGLE_STRIP, HK_E_UNSUPPORTED, "incompatible primitive topology");
  HK_REQUIRE(topology != HK_TOPOLOGY_TRIANGLE_LIST || (n_indices ? n_indices : n_vertices) % 3u == 0u, HK_E_UNSUPPORTED,
             "incompatible primitive topology (index count not a multiple of 3)");
  const uint32_t n_tris = declared_triangles(n_vertices, n_indices, topology);
  HK_REQUIRE(n_tris > 0, HK_E_INVALID, "mesh has no primitive");
  BuilderMesh mesh;
  mesh.vertices.assign(n_vertices, HkVertex{});
  mesh.primitives.assign(n_tris, HkPrimitive{});
  mesh.nodes.reserve(3 * (size_t)n_tris);
  emit_zero_standin(0u, n_tris, mesh.nodes, 0u);
  for (int k = 0; k < 3; ++k) mesh.aabb_center[k] = mesh.aabb_half[k] = 0.0f;
  mesh.pending = true;
  mesh.unresolved = true;
  mesh.decl_indices = n_indices;
  mesh.decl_topology = topology;
  b->meshes.push_back(std::move(mesh));
  b->meshes_dirty = true;
  b->finished = false;
  if (mesh_id) *mesh_id = (uint32_t)b->meshes.size() - 1;
  return HK_OK;
}
int hk_scene_builder_resolve_mesh(hk_scene_builder* b, uint32_t mesh_id, const float* positions, const float* normals, const float* uvs, const uint32_t* indices) {
  HK_REQUIRE(b && positions && normals, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(mesh_id < b->meshes.size() && b->meshes[mesh_id].unresolved, HK_E_INVALID, "mesh %u is not a declared mesh that waits for its arrays", mesh_id);
  const BuilderMesh& m = b->meshes[mesh_id];
  HK_REQUIRE((indices != nullptr) == (m.decl_indices != 0u), HK_E_INVALID, "mesh %u was declared with %u indices: the index array must be %s", mesh_id, m.decl_indices,
             m.decl_indices ? "given" : "NULL");
  const uint32_t nv = (uint32_t)m.vertices.size(), nt = (uint32_t)m.primitives.size(), ni = m.decl_indices ? m.decl_indices : nv;
  for (uint32_t i = 0; indices && i < ni; ++i) HK_REQUIRE(indices[i] < nv, HK_E_INVALID, "vertex index out of range");
  std::vector<HkVertex> vertices(nv);
  for (uint32_t i = 0; i < nv; ++i) {
    HkVertex& v = vertices[i];
    for (int k = 0; k < 3; ++k) {
      v.position[k] = positions[3 * (size_t)i + k];
      v.normal[k] = normals[3 * (size_t)i + k];
    }
    v.u = uvs ? uvs[2 * (size_t)i] : 0.0f;
    v.v = uvs ? uvs[2 * (size_t)i + 1] : 0.0f;
  }
  std::vector<HkPrimitive> primitives(nt);
  const bool strip = m.decl_topology == HK_TOPOLOGY_TRIANGLE_STRIP;
  for (uint32_t t = 0; t < nt; ++t) {  // mod.rs:414-449: a strip's odd triangles flip winding
    const size_t at = strip ? t : 3 * (size_t)t;
    size_t id[3] = {at, at + 1, at + 2};
    if (strip && (t & 1u)) std::swap(id[0], id[1]);
    for (int k = 0; k < 3; ++k) {
      const uint32_t i = indices ? indices[id[k]] : (uint32_t)id[k];
      memcpy(primitives[t].vertices[k].position, vertices[i].position, 12);
      primitives[t].vertices[k].index = i;
    }
  }
  return builder_store_mesh_geometry(b, mesh_id, vertices.data(), nv, primitives.data(), nt, true);
}
int hk_scene_builder_unresolved_meshes(const hk_scene_builder* b, uint32_t* count) {
  HK_REQUIRE(b && count, HK_E_INVALID, "NULL argument");
  *count = builder_unresolved_mesh_count(b);
  return HK_OK;
}

int hk_scene_builder_add_material(hk_scene_builder* b, const HkMaterial* material, uint32_t* material_id) {
  HK_REQUIRE(b && material, HK_E_INVALID, "bad argument");
  b->materials.push_back(*material);
  b->finished = false;
  if (material_id) *material_id = (uint32_t)b->materials.size() - 1;
  return HK_OK;
}

int hk_scene_builder_add_instance(hk_scene_builder* b, uint32_t mesh_id, uint32_t material_id, const float transform[16], uint32_t* instance_id) {
  HK_REQUIRE(b && transform, HK_E_INVALID, "bad argument");
  HK_REQUIRE(mesh_id < b->meshes.size() && material_id < b->materials.size(), HK_E_INVALID, "unknown mesh or material id");
  HK_REQUIRE(!b->meshes[mesh_id].unresolved, HK_E_NOT_READY,
             "mesh %u is declared and not filled yet (hk_scene_builder_declare_mesh): its box is unknown, its instances follow hk_add_meshes_device or hk_scene_builder_resolve_mesh", mesh_id);
  BuilderInstance inst;
  inst.mesh = mesh_id;
  inst.material = material_id;
  memcpy(inst.transform, transform, 64);
  b->instance_decl.push_back(inst);
  b->finished = false;
  if (instance_id) *instance_id = (uint32_t)b->instance_decl.size() - 1;
  return HK_OK;
}

int hk_scene_builder_set_instance_transform(hk_scene_builder* b, uint32_t instance_id, const float transform[16]) {
  HK_REQUIRE(b && transform, HK_E_INVALID, "bad argument");
  HK_REQUIRE(instance_id < b->instance_decl.size(), HK_E_INVALID, "unknown instance id");
  memcpy(b->instance_decl[instance_id].transform, transform, 64);
  b->finished = false;
  return HK_OK;
}

// The host twin of the device refit (mesh_deform.hip): same topology, every navigator box the union of the triangle boxes below it -
// a triangle's box with the leaf-box arithmetic of the device layout (scene_layout.hip build_static_region: IEEE min / max with -0 < +0),
// the union of two children as std::min / std::max of (first child, second child), as kernels_tree.hip k_lbvh_boxes forms it.
namespace {
float leaf_min(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? a : b;
  return a < b ? a : b;
}
float leaf_max(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? b : a;
  return a > b ? a : b;
}
// every navigator box of a flatten_custom array refit, back to front (a navigator's subtree lies behind it: no recursion, whatever the
// depth); false if the array is not in that layout
bool refit_nodes(std::vector<HkNode>& nodes, const std::vector<HkPrimitive>& prims) {
  const uint32_t n = (uint32_t)nodes.size();
  if (n == 0) return false;
  auto leaf = [&](uint32_t i) { return nodes[i].entry_index >= HK_BVH_LEAF_FLAG; };
  if (n == 1) return leaf(0) && nodes[0].entry_index - HK_BVH_LEAF_FLAG < prims.size();
  if (leaf(0) || nodes[0].exit_index >= n || nodes[nodes[0].exit_index].exit_index != n) return false;
  std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);  // the box of the subtree that starts at node i
  for (uint32_t i = n; i-- > 0;) {
    HkNode& nd = nodes[i];
    if (leaf(i)) {
      if (nd.entry_index - HK_BVH_LEAF_FLAG >= prims.size() || nd.exit_index != i + 1) return false;
      const HkPrimitiveVertex* v = prims[nd.entry_index - HK_BVH_LEAF_FLAG].vertices;
      for (int k = 0; k < 3; ++k) {
        lo[3 * i + k] = leaf_min(v[0].position[k], leaf_min(v[1].position[k], v[2].position[k]));
        hi[3 * i + k] = leaf_max(v[0].position[k], leaf_max(v[1].position[k], v[2].position[k]));
      }
      continue;
    }
    const uint32_t a = i + 1, e = nd.exit_index;  // the subtree [a, e): one leaf, or [navigator a][..][navigator bb][..]
    if (nd.entry_index != a || !(e > a && e <= n)) return false;
    if (leaf(a)) {
      if (e != a + 1) return false;
      for (int k = 0; k < 3; ++k) { lo[3 * i + k] = lo[3 * a + k]; hi[3 * i + k] = hi[3 * a + k]; }
    } else {
      const uint32_t bb = nodes[a].exit_index;
      if (!(bb > a + 1 && bb < e) || leaf(bb) || nodes[bb].entry_index != bb + 1 || nodes[bb].exit_index != e) return false;
      for (int k = 0; k < 3; ++k) {
        lo[3 * i + k] = std::min(lo[3 * a + k], lo[3 * bb + k]);
        hi[3 * i + k] = std::max(hi[3 * a + k], hi[3 * bb + k]);
      }
    }
    memcpy(nd.min, &lo[3 * i], 12);
    memcpy(nd.max, &hi[3 * i], 12);
  }
  return true;
}
}  // namespace

int hk_scene_builder_set_mesh_vertices(hk_scene_builder* b, uint32_t mesh_id, const float* positions, const float* normals) {
  HK_REQUIRE(b && positions, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  HK_NO_UNRESOLVED_MESH(b, mesh_id);
  BuilderMesh mesh = b->meshes[mesh_id];  // (a copy: an error leaves the builder as it was)
  for (size_t i = 0; i < mesh.vertices.size(); ++i)
    for (int k = 0; k < 3; ++k) {
      mesh.vertices[i].position[k] = positions[3 * i + k];
      if (normals) mesh.vertices[i].normal[k] = normals[3 * i + k];
    }
  for (HkPrimitive& p : mesh.primitives)
    for (int k = 0; k < 3; ++k) memcpy(p.vertices[k].position, mesh.vertices[p.vertices[k].index].position, 12);
  HK_REQUIRE(refit_nodes(mesh.nodes, mesh.primitives), HK_E_UNSUPPORTED, "the mesh tree is not in the flatten_custom layout");
  float mn[3], mx[3];
  // the mesh box over all vertices, as the device reduces it (order-free: -0 < +0)
  for (int k = 0; k < 3; ++k) mn[k] = mx[k] = mesh.vertices[0].position[k];
  for (const HkVertex& v : mesh.vertices)
    for (int k = 0; k < 3; ++k) {
      mn[k] = leaf_min(mn[k], v.position[k]);
      mx[k] = leaf_max(mx[k], v.position[k]);
    }
  for (int k = 0; k < 3; ++k) {  // bevy Aabb::from_min_max
    mesh.aabb_center[k] = 0.5f * (mx[k] + mn[k]);
    mesh.aabb_half[k] = 0.5f * (mx[k] - mn[k]);
  }
  b->meshes[mesh_id] = std::move(mesh);
  b->concat_meshes = std::min<size_t>(b->concat_meshes, mesh_id);
  b->meshes_dirty = true;
  b->finished = false;
  return HK_OK;
}

// The host twin of HK_DEFORM_RECOMPUTE_NORMALS (kernels_deform.hip k_deform_triangles' face vectors, k_deform_normals' gather): the same
// f32 operations in the same order (no contraction: -ffp-contract=off), so the normals equal the device's bit for bit.
int hk_scene_builder_recompute_mesh_normals(hk_scene_builder* b, uint32_t mesh_id) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_REQUIRE(mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  HK_NO_UNRESOLVED_MESH(b, mesh_id);
  BuilderMesh& mesh = b->meshes[mesh_id];
  const size_t nv = mesh.vertices.size();
  for (const HkPrimitive& p : mesh.primitives)
    for (int k = 0; k < 3; ++k) HK_REQUIRE(p.vertices[k].index < nv, HK_E_INVALID, "a triangle names vertex %u of %zu", p.vertices[k].index, nv);
  std::vector<float> sum(3 * nv, 0.0f);  // (+0: the first face vector is added to it, so a sum of -0 stores +0)
  for (const HkPrimitive& p : mesh.primitives) {  // ascending triangle, then corner: every vertex's sum in the order of the rule
    const float* p0 = mesh.vertices[p.vertices[0].index].position;
    const float* p1 = mesh.vertices[p.vertices[1].index].position;
    const float* p2 = mesh.vertices[p.vertices[2].index].position;
    const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const float f[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    for (int k = 0; k < 3; ++k) {
      float* s = &sum[3 * (size_t)p.vertices[k].index];
      for (int a = 0; a < 3; ++a) s[a] = s[a] + f[a];
    }
  }
  for (size_t v = 0; v < nv; ++v) {
    const float* s = &sum[3 * v];
    if (s[0] == 0.0f && s[1] == 0.0f && s[2] == 0.0f) continue;  // (also a vertex no triangle names: it keeps its normal)
    memcpy(mesh.vertices[v].normal, s, 12);
  }
  b->concat_meshes = std::min<size_t>(b->concat_meshes, mesh_id);
  b->meshes_dirty = true;
  b->finished = false;
  return HK_OK;
}

// The host twin of the device rebuild (mesh_deform.hip hk_rebuild_mesh_tree, HK_TREE_SAH): the tree hk_scene_builder_add_mesh would
// build over the mesh's CURRENT triangles - `bvh` 0.7.1 BVH::build over their boxes, formed with add_mesh's arithmetic - and then the
// canonical navigator boxes of refit_nodes, so that the result is what the device writes and what a later refit leaves alone.
static int canonical_mesh_tree(const BuilderMesh& mesh, std::vector<HkNode>& nodes) {
  std::vector<float> boxes;
  boxes.reserve(mesh.primitives.size() * 6);
  for (const HkPrimitive& p : mesh.primitives) {
    Box bx = Box::empty();
    for (int k = 0; k < 3; ++k) bx.grow(p.vertices[k].position);
    boxes.insert(boxes.end(), bx.mn, bx.mn + 3);
    boxes.insert(boxes.end(), bx.mx, bx.mx + 3);
  }
  nodes = build_flat_bvh(boxes);
  HK_REQUIRE(nodes.size() == mesh.nodes.size() && refit_nodes(nodes, mesh.primitives), HK_E_UNSUPPORTED, "the rebuilt mesh tree is not in the flatten_custom layout");
  return HK_OK;
}
int hk_scene_builder_rebuild_mesh_tree(hk_scene_builder* b, uint32_t mesh_id) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_REQUIRE(mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  HK_NO_UNRESOLVED_MESH(b, mesh_id);
  std::vector<HkNode> nodes;  // (a copy: an error leaves the builder as it was)
  const int rc = canonical_mesh_tree(b->meshes[mesh_id], nodes);
  if (rc) return rc;
  b->meshes[mesh_id].nodes.swap(nodes);
  b->meshes[mesh_id].pending = false;  // (a deferred mesh: this is its tree)
  b->concat_meshes = std::min<size_t>(b->concat_meshes, mesh_id);
  b->meshes_dirty = true;
  b->finished = false;
  return HK_OK;
}

// The host completion of the deferred meshes (hk_scene_builder_add_mesh_deferred): per pending mesh the tree of
// hk_scene_builder_rebuild_mesh_tree, written over the stand-in IN PLACE - the mesh's own nodes and, in a finished builder, its range of
// the concatenated array; the node count does not depend on the tree, so no offset moves and a finished builder stays finished.
int hk_scene_builder_build_pending_mesh_trees(hk_scene_builder* b) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_NO_UNRESOLVED_MESHES(b);  // (before the first tree: a refusal writes nothing)
  for (uint32_t id = 0; id < b->meshes.size(); ++id) {
    if (!b->meshes[id].pending) continue;
    const int rc = builder_complete_mesh_on_host(b, id);
    if (rc) return rc;
  }
  return HK_OK;
}

int hk_scene_builder_mesh_index(const hk_scene_builder* b, uint32_t mesh_id, HkMeshIndex* out) {
  HK_REQUIRE(b && out, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(!b->meshes_dirty && mesh_id < b->mesh_index.size(), HK_E_INVALID, "unknown mesh id, or the builder was not finished since the mesh was added");
  *out = b->mesh_index[mesh_id];
  return HK_OK;
}

static int finish_impl(hk_scene_builder* b, bool build_trees);
int hk_scene_builder_finish(hk_scene_builder* b) { return finish_impl(b, true); }
int hk_scene_builder_finish_instances(hk_scene_builder* b) { return finish_impl(b, false); }

int hk_scene_builder_remove_instance(hk_scene_builder* b, uint32_t instance_id) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_REQUIRE(instance_id < b->instance_decl.size(), HK_E_INVALID, "unknown instance id");
  b->instance_decl.erase(b->instance_decl.begin() + instance_id);
  // the transform history is kept per instance: the rows of the removed one go with it
  for (std::vector<float>* v : {&b->finished_transforms, &b->previous_transforms})
    if (v->size() >= 16 * ((size_t)instance_id + 1)) v->erase(v->begin() + 16 * (size_t)instance_id, v->begin() + 16 * ((size_t)instance_id + 1));
  b->finished = false;
  return HK_OK;
}

int hk_scene_builder_mesh_extent(const hk_scene_builder* b, uint32_t mesh_id, HkMeshExtent* out) {
  HK_REQUIRE(b && out, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  *out = mesh_id < b->last_extent.size() ? b->last_extent[mesh_id] : HkMeshExtent{0u, 0u, 0u, 0u, 0u, 0u};  // (no finish has seen it: it lies in no array)
  return HK_OK;
}

int hk_scene_builder_remove_mesh(hk_scene_builder* b, uint32_t mesh_id, HkMeshExtent* removed) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_REQUIRE(mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  for (size_t i = 0; i < b->instance_decl.size(); ++i)
    HK_REQUIRE(b->instance_decl[i].mesh != mesh_id, HK_E_INVALID, "instance %zu still names mesh %u: remove its instances first (hk_scene_builder_remove_instance)", i, mesh_id);
  // ---- nothing is refused from here on
  if (removed) (void)hk_scene_builder_mesh_extent(b, mesh_id, removed);
  if (mesh_id < b->last_extent.size()) b->last_extent.erase(b->last_extent.begin() + mesh_id);
  // the concatenated arrays end where the removed mesh began: the next finish appends the meshes behind it again, what lies in front
  // keeps its bytes
  if (mesh_id < b->mesh_index.size()) {
    const HkMeshIndex cut = b->mesh_index[mesh_id];
    b->vertices.resize(cut.vertex); b->primitives.resize(cut.primitive); b->asset_nodes.resize(cut.node_offset);
    b->mesh_index.resize(mesh_id);
  }
  b->meshes.erase(b->meshes.begin() + mesh_id);
  for (hk::BuilderInstance& d : b->instance_decl)
    if (d.mesh > mesh_id) d.mesh -= 1;
  b->concat_meshes = std::min<size_t>(b->concat_meshes, mesh_id);
  b->meshes_dirty = true;
  b->finished = false;
  return HK_OK;
}

int hk_rebase_mesh_index(const HkMeshExtent* removed, uint32_t n, const HkMeshIndex* index, HkMeshIndex* out) {
  HK_REQUIRE((removed || !n) && index && out, HK_E_INVALID, "NULL argument");
  // per range the number of removed elements in front of the value: an extent that begins in front of it counts up to the value
  auto gone = [](uint32_t at, uint32_t begin, uint32_t count) { return begin < at ? std::min(count, at - begin) : 0u; };
  HkMeshIndex r = *index;
  for (uint32_t k = 0; k < n; ++k) {
    const HkMeshExtent& e = removed[k];
    if (!e.node_count) continue;  // (a mesh no finish had seen: it lay in no array)
    r.vertex -= gone(index->vertex, e.vertex, e.n_vertices);
    r.primitive -= gone(index->primitive, e.primitive, e.n_primitives);
    r.node_offset -= gone(index->node_offset, e.node_offset, e.node_count);
  }
  *out = r;
  return HK_OK;
}

int hk_scene_builder_set_instance_material(hk_scene_builder* b, uint32_t instance_id, uint32_t material_id) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  HK_REQUIRE(instance_id < b->instance_decl.size() && material_id < b->materials.size(), HK_E_INVALID, "unknown instance or material id");
  b->instance_decl[instance_id].material = material_id;
  b->finished = false;
  return HK_OK;
}

int hk_scene_builder_set_material(hk_scene_builder* b, uint32_t material_id, const HkMaterial* material) {
  HK_REQUIRE(b && material, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(material_id < b->materials.size(), HK_E_INVALID, "unknown material id");
  b->materials[material_id] = *material;
  b->finished = false;
  return HK_OK;
}

static int finish_impl(hk_scene_builder* b, bool build_trees) {
  HK_REQUIRE(b, HK_E_INVALID, "builder is NULL");
  if (b->meshes_dirty) {  // mesh.rs:141-163: concatenate, remember offsets (only when a mesh was added)
    // The reference concatenates every mesh again; the bytes in front of the first mesh that changed are what they were, so the work here
    // starts there: meshes added since the last finish are appended, at a cost that follows them.
    const size_t keep = std::min(b->concat_meshes, b->mesh_index.size());
    if (keep < b->mesh_index.size()) {
      const HkMeshIndex& cut = b->mesh_index[keep];
      b->vertices.resize(cut.vertex); b->primitives.resize(cut.primitive); b->asset_nodes.resize(cut.node_offset);
      b->mesh_index.resize(keep);
    }
    for (size_t id = keep; id < b->meshes.size(); ++id) {
      const BuilderMesh& m = b->meshes[id];
      HkMeshIndex mi;
      mi.vertex = (uint32_t)b->vertices.size();
      mi.primitive = (uint32_t)b->primitives.size();
      mi.node_offset = (uint32_t)b->asset_nodes.size();
      mi.node_count = (uint32_t)m.nodes.size();
      b->vertices.insert(b->vertices.end(), m.vertices.begin(), m.vertices.end());
      b->primitives.insert(b->primitives.end(), m.primitives.begin(), m.primitives.end());
      b->asset_nodes.insert(b->asset_nodes.end(), m.nodes.begin(), m.nodes.end());
      b->mesh_index.push_back(mi);
    }
    b->concat_meshes = b->meshes.size();
    b->meshes_dirty = false;
    b->last_extent.resize(b->meshes.size());
    for (size_t id = 0; id < b->meshes.size(); ++id) {
      const HkMeshIndex& mi = b->mesh_index[id];
      b->last_extent[id] = HkMeshExtent{mi.vertex, (uint32_t)b->meshes[id].vertices.size(), mi.primitive, (uint32_t)b->meshes[id].primitives.size(), mi.node_offset, mi.node_count};
    }
  }
  b->instances.clear(); b->instance_nodes.clear(); b->emissives.clear(); b->emissive_nodes.clear(); b->alias_table.clear();
  builder_commit_transforms(b);  // PreviousMeshUniform: what the transforms were at the last finish (new instances: their own)
  // instance.rs:286-325
  std::vector<float> boxes;
  for (const BuilderInstance& d : b->instance_decl) {
    const BuilderMesh& mesh = b->meshes[d.mesh];
    HkInstance inst;
    memset(&inst, 0, sizeof(inst));
    HK_REQUIRE(instance_world_record(d.transform, mesh.aabb_center, mesh.aabb_half, inst.min, inst.max, inst.inverse_transpose_model), HK_E_INVALID,
               "singular instance transform");
    inst.material = d.material;
    memcpy(inst.model, d.transform, 64);
    inst.mesh = b->mesh_index[d.mesh];
    b->instances.push_back(inst);
    boxes.insert(boxes.end(), inst.min, inst.min + 3);
    boxes.insert(boxes.end(), inst.max, inst.max + 3);
  }
  b->instance_nodes = build_trees ? build_flat_bvh(boxes) : build_flat_placeholder(boxes);  // instance.rs:365-371
  // `BHShape::set_bh_node_index` bookkeeping (unused by the shaders): position of the leaf node
  for (uint32_t n = 0; n < b->instance_nodes.size(); ++n)
    if (b->instance_nodes[n].entry_index >= HK_BVH_LEAF_FLAG) b->instances[b->instance_nodes[n].entry_index - HK_BVH_LEAF_FLAG].node_index = n;

  // instance.rs:380-420: emissive list, alias tables
  std::vector<float> eboxes;
  for (uint32_t id = 0; id < b->instances.size(); ++id) {
    const HkInstance& inst = b->instances[id];
    const HkMaterial& mat = b->materials[inst.material];
    const float* e = mat.emissive;
    float intensity = emissive_intensity(e);
    if (!(intensity > 0.0f)) continue;
    const BuilderMesh& mesh = b->meshes[b->instance_decl[id].mesh];
    std::vector<float> areas = primitive_areas(mesh, inst.model);
    std::vector<HkAliasEntry> table = build_alias_table(areas);
    HkEmissive em;
    memset(&em, 0, sizeof(em));
    memcpy(em.emissive, e, 16);
    float d2 = 0.0f;
    for (int k = 0; k < 3; ++k) {
      em.position[k] = 0.5f * (inst.max[k] + inst.min[k]);
      float d = inst.max[k] - inst.min[k];
      d2 += d * d;
    }
    em.radius = 0.5f * sqrtf(d2) + sqrtf(intensity);
    em.instance = id;
    em.alias_table[0] = (uint32_t)b->alias_table.size();
    em.alias_table[1] = (uint32_t)table.size();
    b->alias_table.insert(b->alias_table.end(), table.begin(), table.end());
    float area = 0.0f;
    for (float a : areas) area += a;
    em.surface_area = area;
    b->emissives.push_back(em);
    for (int k = 0; k < 3; ++k) eboxes.push_back(em.position[k] - em.radius);
    for (int k = 0; k < 3; ++k) eboxes.push_back(em.position[k] + em.radius);
  }
  b->emissive_nodes = build_trees ? build_flat_bvh(eboxes) : build_flat_placeholder(eboxes);  // instance.rs:422-428
  for (uint32_t n = 0; n < b->emissive_nodes.size(); ++n)
    if (b->emissive_nodes[n].entry_index >= HK_BVH_LEAF_FLAG) b->emissives[b->emissive_nodes[n].entry_index - HK_BVH_LEAF_FLAG].node_index = n;
  b->finished = true;
  b->standin_trees = !build_trees && (b->instances.size() > 1 || b->emissives.size() > 1);  // (a tree of one leaf has one shape)
  return HK_OK;
}

#define HK_BUILDER_GETTER(name, field, type)                                                   \
  int hk_scene_builder_##name(const hk_scene_builder* b, const type** p, uint32_t* n) {        \
    HK_REQUIRE(b && p && n, HK_E_INVALID, "bad argument");                                     \
    HK_REQUIRE(b->finished, HK_E_NOT_READY, "call hk_scene_builder_finish first");             \
    *p = b->field.data();                                                                      \
    *n = (uint32_t)b->field.size();                                                            \
    return HK_OK;                                                                              \
  }
HK_BUILDER_GETTER(vertices, vertices, HkVertex)
HK_BUILDER_GETTER(primitives, primitives, HkPrimitive)
HK_BUILDER_GETTER(asset_nodes, asset_nodes, HkNode)
HK_BUILDER_GETTER(materials, materials, HkMaterial)
HK_BUILDER_GETTER(instances, instances, HkInstance)
HK_BUILDER_GETTER(instance_nodes, instance_nodes, HkNode)
HK_BUILDER_GETTER(emissives, emissives, HkEmissive)
HK_BUILDER_GETTER(emissive_nodes, emissive_nodes, HkNode)
HK_BUILDER_GETTER(alias_table, alias_table, HkAliasEntry)

int hk_scene_builder_previous_transforms(const hk_scene_builder* b, const float** p, uint32_t* n) {
  HK_REQUIRE(b && p && n, HK_E_INVALID, "bad argument");
  HK_REQUIRE(b->finished, HK_E_NOT_READY, "call hk_scene_builder_finish first");
  *p = b->previous_transforms.data();
  *n = (uint32_t)(b->previous_transforms.size() / 16);
  return HK_OK;
}

}  // extern "C"

namespace hk {
uint32_t builder_pending_mesh_count(const hk_scene_builder* b) {
  uint32_t n = 0;
  if (b)
    for (const BuilderMesh& m : b->meshes) n += m.pending ? 1u : 0u;
  return n;
}
bool builder_pending_mesh(const hk_scene_builder* b, uint32_t mesh_id, HkMeshIndex* index) {
  if (!b || mesh_id >= b->meshes.size() || !b->meshes[mesh_id].pending) return false;
  if (index && !b->meshes_dirty && mesh_id < b->mesh_index.size()) *index = b->mesh_index[mesh_id];
  return true;
}
uint32_t builder_mesh_count(const hk_scene_builder* b) { return b ? (uint32_t)b->meshes.size() : 0u; }
uint32_t builder_unresolved_mesh_count(const hk_scene_builder* b, uint32_t* first) {
  uint32_t n = 0;
  if (b)
    for (size_t id = b->meshes.size(); id-- > 0;)
      if (b->meshes[id].unresolved) {
        n += 1u;
        if (first) *first = (uint32_t)id;
      }
  return n;
}
bool builder_unresolved_mesh(const hk_scene_builder* b, uint32_t mesh_id, DeclaredMesh* out) {
  if (!b || mesh_id >= b->meshes.size() || !b->meshes[mesh_id].unresolved) return false;
  const BuilderMesh& m = b->meshes[mesh_id];
  if (out) *out = DeclaredMesh{(uint32_t)m.vertices.size(), (uint32_t)m.primitives.size(), m.decl_indices, m.decl_topology};
  return true;
}
// what fills a declared mesh, whoever assembled the records (hk_scene_builder_resolve_mesh on the host, hk_add_meshes_device's kernel): the
// mesh's own arrays and, in a finished builder, its ranges of the concatenated ones in place - the counts are the declaration's, so no
// offset moves and a finished builder stays finished; the mesh box with add_mesh's arithmetic over ALL vertices; `standin`: the deferred
// mesh's stand-in over the real triangle boxes (a caller that builds the tree at once leaves the declaration's).  Clears `unresolved`.
int builder_store_mesh_geometry(hk_scene_builder* b, uint32_t mesh_id, const HkVertex* vertices, uint32_t n_vertices, const HkPrimitive* primitives, uint32_t n_primitives,
                                bool standin) {
  HK_REQUIRE(b && vertices && primitives && mesh_id < b->meshes.size() && b->meshes[mesh_id].unresolved, HK_E_INVALID, "mesh %u is not a declared mesh that waits for its arrays",
             mesh_id);
  BuilderMesh& m = b->meshes[mesh_id];
  HK_REQUIRE(n_vertices == m.vertices.size() && n_primitives == m.primitives.size(), HK_E_INVALID, "%u vertices and %u triangles for a mesh declared with %zu and %zu", n_vertices,
             n_primitives, m.vertices.size(), m.primitives.size());
  std::vector<HkNode> standin_nodes;  // (before anything is written: a refusal leaves the mesh as it was)
  if (standin) {
    std::vector<float> boxes;
    boxes.reserve((size_t)n_primitives * 6);
    for (uint32_t t = 0; t < n_primitives; ++t) {
      Box bx = Box::empty();
      for (int k = 0; k < 3; ++k) bx.grow(primitives[t].vertices[k].position);
      boxes.insert(boxes.end(), bx.mn, bx.mn + 3);
      boxes.insert(boxes.end(), bx.mx, bx.mx + 3);
    }
    standin_nodes = build_flat_placeholder(boxes);
    HK_REQUIRE(standin_nodes.size() == m.nodes.size(), HK_E_INVALID, "a stand-in of %zu nodes for a mesh of %zu", standin_nodes.size(), m.nodes.size());
  }
  std::copy(vertices, vertices + n_vertices, m.vertices.begin());
  std::copy(primitives, primitives + n_primitives, m.primitives.begin());
  float mn[3], mx[3];
  for (int k = 0; k < 3; ++k) mn[k] = mx[k] = vertices[0].position[k];
  for (uint32_t i = 0; i < n_vertices; ++i)
    for (int k = 0; k < 3; ++k) {
      mn[k] = std::min(mn[k], vertices[i].position[k]);
      mx[k] = std::max(mx[k], vertices[i].position[k]);
    }
  for (int k = 0; k < 3; ++k) {  // bevy Aabb::from_min_max
    m.aabb_center[k] = 0.5f * (mx[k] + mn[k]);
    m.aabb_half[k] = 0.5f * (mx[k] - mn[k]);
  }
  if (standin) m.nodes.swap(standin_nodes);
  m.unresolved = false;
  const bool in_place = mesh_id < b->concat_meshes && mesh_id < b->mesh_index.size();
  if (in_place) {
    const HkMeshIndex& mi = b->mesh_index[mesh_id];
    if (mi.node_count == m.nodes.size() && (size_t)mi.node_offset + mi.node_count <= b->asset_nodes.size() && (size_t)mi.vertex + n_vertices <= b->vertices.size() &&
        (size_t)mi.primitive + n_primitives <= b->primitives.size()) {
      std::copy(vertices, vertices + n_vertices, b->vertices.begin() + mi.vertex);
      std::copy(primitives, primitives + n_primitives, b->primitives.begin() + mi.primitive);
      if (standin) std::copy(m.nodes.begin(), m.nodes.end(), b->asset_nodes.begin() + mi.node_offset);
      return HK_OK;
    }
  }
  b->concat_meshes = std::min<size_t>(b->concat_meshes, mesh_id);  // (the next finish concatenates again from this mesh on)
  if (!b->meshes_dirty) {
    b->meshes_dirty = true;
    b->finished = false;
  }
  return HK_OK;
}
int builder_store_mesh_nodes(hk_scene_builder* b, uint32_t mesh_id, const HkNode* nodes, uint32_t count) {
  HK_REQUIRE(b && nodes && mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  BuilderMesh& m = b->meshes[mesh_id];
  HK_REQUIRE(count == m.nodes.size(), HK_E_INVALID, "a tree of %u nodes for a mesh of %zu", count, m.nodes.size());
  std::copy(nodes, nodes + count, m.nodes.begin());
  // the mesh's range of the concatenated array, where that array still holds the mesh as it stands (whether or not meshes were added
  // since); otherwise the next finish concatenates again from this mesh on
  if (mesh_id < b->concat_meshes && mesh_id < b->mesh_index.size() && b->mesh_index[mesh_id].node_count == count &&
      (size_t)b->mesh_index[mesh_id].node_offset + count <= b->asset_nodes.size())
    std::copy(nodes, nodes + count, b->asset_nodes.begin() + b->mesh_index[mesh_id].node_offset);
  else
    b->concat_meshes = std::min<size_t>(b->concat_meshes, mesh_id);
  m.pending = false;
  return HK_OK;
}
int builder_complete_mesh_on_host(hk_scene_builder* b, uint32_t mesh_id) {
  HK_REQUIRE(b && mesh_id < b->meshes.size(), HK_E_INVALID, "unknown mesh id");
  HK_NO_UNRESOLVED_MESH(b, mesh_id);
  std::vector<HkNode> nodes;
  const int rc = canonical_mesh_tree(b->meshes[mesh_id], nodes);
  if (rc) return rc;
  return builder_store_mesh_nodes(b, mesh_id, nodes.data(), (uint32_t)nodes.size());
}
}  // namespace hk
