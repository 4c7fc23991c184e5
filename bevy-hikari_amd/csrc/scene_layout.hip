// scene_layout.hip - uploads and the layout conversion behind them: the reference-layout scene arrays a host hands over
// (src/mesh_material/mesh.rs:43-64, material.rs:201-202, instance.rs:82-108, src/lib.rs:189-219) become the device's scene blob -
// SoA node / triangle / vertex planes, leaf boxes filled in, navigators folded, direction-threaded orderings, the one-level tree of
// scenes under one transform, two slots of the instance-level region with asynchronous updates.
#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

namespace {
__global__ void k_copy_u4(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

}  // namespace

namespace hk {
// `bvh` 0.7.1's flat format puts a "navigator" node (child box, entry = next) in front of EVERY subtree,
// including single-leaf subtrees, and the reference then tests the leaf's own (re-derived) box again:
// two steps with the same box for every leaf reached.  With leaf boxes filled in at upload, a navigator
// whose subtree is one leaf with an equal box can take over the leaf's role (entry := leaf entry): the
// walk performs box test -> leaf action -> continue at the same exit index, i.e. exactly the outcomes
// of the two-step sequence, and the original leaf slot is simply never visited.  No index changes.
// entry/exit are LOCAL to [begin, begin + count).  Returns the number of folded navigators.
size_t fold_leaf_navigators(std::vector<float4>& lo, std::vector<float4>& hi, size_t begin, size_t count) {
  auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
  size_t folded = 0;
  for (size_t k = 0; k + 1 < count; ++k) {
    float4& nlo = lo[begin + k];
    const float4& nhi = hi[begin + k];
    const uint32_t entry = bits(nlo.w), exit_ = bits(nhi.w);
    if (entry >= HK_BVH_LEAF_FLAG || entry != k + 1) continue;
    const float4& clo = lo[begin + k + 1];
    const float4& chi = hi[begin + k + 1];
    if (bits(clo.w) < HK_BVH_LEAF_FLAG || bits(chi.w) != exit_) continue;
    if (!(nlo.x == clo.x && nlo.y == clo.y && nlo.z == clo.z && nhi.x == chi.x && nhi.y == chi.y && nhi.z == chi.z)) continue;
    nlo.w = clo.w;
    ++folded;
  }
  return folded;
}

// Convert the reference-layout scene to the device layout (hk_device.hpp header comment).
//
// One device allocation, two regions:
//   [ instance-level region, `dyn_capacity` bytes ][ mesh-level region, `mesh.bytes` bytes ]
// The instance-level region (TLAS nodes first, instances, light BVH, emissives, alias tables,
// materials, texture descriptors) is what prepare_instances / prepare_material_assets rewrite when
// something moves (instance.rs:352-437); it is small (0.6 MB at 2 000 instances) and is the only part
// rebuilt and re-sent for an instance-only change.  The mesh-level region (BLAS nodes with their leaf
// boxes, triangle planes, vertex planes) changes only with the mesh assets (mesh.rs:106-166).
// Node indices are in 32-B units from the start of the allocation: TLAS node i is node i, BLAS node k
// of a mesh is node blas_base + node_offset + k with blas_base = dyn_capacity / 32.

// `orderings` flattenings of the reference-layout array `src` (ordering 0 = the reference's own order), each range
// [offset, offset + count) of `ranges` re-threaded on its own (hk_bvh_rethread); a malformed range keeps the reference order
void thread_orderings(const std::vector<HkNode>& src, const std::vector<std::pair<uint32_t, uint32_t>>& ranges, int orderings, std::vector<std::vector<HkNode>>& out) {
  out.assign((size_t)orderings, std::vector<HkNode>());
  out[0] = src;
  if (orderings <= 1) return;
  auto rethread = [&](int o) {
    for (const auto& r : ranges)
      if (r.second && !rethread_flat_bvh(src.data() + r.first, r.second, (uint32_t)o, out[o].data() + r.first))
        std::copy(src.begin() + r.first, src.begin() + r.first + r.second, out[o].begin() + r.first);
  };
  for (int o = 1; o < orderings; ++o) out[o] = src;
  // Small trees (the instance tree of an animated frame, a few thousand nodes) are re-threaded on the calling thread: spawning
  // seven threads costs more than the work and sits on the per-frame path.  Large mesh trees use worker threads; a thread that
  // cannot be created, or a worker that throws (bad_alloc), must not escape through the extern "C" boundary: the orderings it did
  // not produce are redone serially here.
  size_t total = 0;
  for (const auto& r : ranges) total += r.second;
  std::vector<uint8_t> done((size_t)orderings, 0);
  if (total >= 8192) {
    std::vector<std::thread> workers;
    try {
      for (int o = 1; o < orderings; ++o)
        workers.emplace_back([&, o]() {
          try {
            rethread(o);
            done[(size_t)o] = 1;
          } catch (...) {
          }
        });
    } catch (...) {
    }
    for (std::thread& w : workers) w.join();
  }
  for (int o = 1; o < orderings; ++o)
    if (!done[(size_t)o]) {
      out[o] = src;
      rethread(o);
    }
}

// mesh-level region; fills c->node_prim_offset.  Needs the instances' mesh records to know which
// primitive range a BLAS leaf indexes (GpuMeshIndex travels with the instance, mod.rs:147-156).  `mesh`: the region the blob holds, exact.
int build_static_region(hk_ctx* c, Blob& blob, MeshRegion& mesh) {
  const size_t n_nodes = c->asset_nodes.size(), n_prims = c->primitives.size(), n_verts = c->vertices.size();
  std::vector<int64_t>& node_prim_offset = c->node_prim_offset;
  node_prim_offset.assign(n_nodes, -1);
  for (const HkInstance& in : c->instances)
    for (uint32_t k = 0; k < in.mesh.node_count; ++k) node_prim_offset[in.mesh.node_offset + k] = in.mesh.primitive;
  std::vector<std::pair<uint32_t, uint32_t>> ranges;  // distinct mesh ranges
  {
    std::vector<uint8_t> done(n_nodes + 1, 0);
    for (const auto& r : c->load_pending_ranges)  // (hk_load_scene: stand-ins the device overwrites in every ordering)
      if (r.first < n_nodes) done[r.first] = 1;
    for (const HkInstance& in : c->instances) {
      if (in.mesh.node_count == 0 || done[in.mesh.node_offset]) continue;
      done[in.mesh.node_offset] = 1;
      ranges.emplace_back(in.mesh.node_offset, in.mesh.node_count);
    }
  }
  const int orderings = c->threaded ? 8 : 1;
  std::vector<std::vector<HkNode>> ordered;
  thread_orderings(c->asset_nodes, ranges, orderings, ordered);
  std::vector<float4> nodes;
  nodes.reserve(2 * n_nodes * (size_t)orderings);
  std::vector<float4> lo(n_nodes), hi(n_nodes);
  for (int o = 0; o < orderings; ++o) {
    const std::vector<HkNode>& src = ordered[o];
    for (size_t i = 0; i < n_nodes; ++i) {
      const HkNode& n = src[i];
      float mn[3] = {n.min[0], n.min[1], n.min[2]}, mx[3] = {n.max[0], n.max[1], n.max[2]};
      if (n.entry_index >= HK_BVH_LEAF_FLAG && node_prim_offset[i] >= 0) {  // light.wgsl:408-412
        size_t prim = (size_t)node_prim_offset[i] + (n.entry_index - HK_BVH_LEAF_FLAG);
        HK_REQUIRE(prim < n_prims, HK_E_INVALID, "BLAS leaf primitive out of bounds");
        const HkPrimitiveVertex* v = c->primitives[prim].vertices;
        for (int k = 0; k < 3; ++k) {
          mn[k] = hmin(v[0].position[k], hmin(v[1].position[k], v[2].position[k]));
          mx[k] = hmax(v[0].position[k], hmax(v[1].position[k], v[2].position[k]));
        }
      }
      lo[i] = make_float4(mn[0], mn[1], mn[2], as_f(n.entry_index));
      hi[i] = make_float4(mx[0], mx[1], mx[2], as_f(n.exit_index));
    }
    for (const auto& r : ranges) fold_leaf_navigators(lo, hi, r.first, r.second);  // fold single-leaf navigators, once per distinct mesh range
    for (size_t i = 0; i < n_nodes; ++i) { nodes.push_back(lo[i]); nodes.push_back(hi[i]); }
  }
  mesh.nodes = blob.add(nodes);  // offset 0: the region itself starts on a 32-B boundary

  std::vector<float4> v0(n_prims), v1(n_prims), v2(n_prims);
  for (size_t i = 0; i < n_prims; ++i) {
    const HkPrimitiveVertex* v = c->primitives[i].vertices;
    v0[i] = make_float4(v[0].position[0], v[0].position[1], v[0].position[2], as_f(v[0].index));
    v1[i] = make_float4(v[1].position[0], v[1].position[1], v[1].position[2], as_f(v[1].index));
    v2[i] = make_float4(v[2].position[0], v[2].position[1], v[2].position[2], as_f(v[2].index));
  }
  mesh.v0 = blob.add(v0); mesh.v1 = blob.add(v1); mesh.v2 = blob.add(v2);
  std::vector<float4> vn(n_verts);
  std::vector<float2> vuv(n_verts);
  for (size_t i = 0; i < n_verts; ++i) {
    vn[i] = make_float4(c->vertices[i].normal[0], c->vertices[i].normal[1], c->vertices[i].normal[2], 0.0f);
    vuv[i] = make_float2(c->vertices[i].u, c->vertices[i].v);
  }
  mesh.vn = blob.add(vn); mesh.vuv = blob.add(vuv);
  blob.bytes.resize((blob.bytes.size() + 15) & ~(size_t)15, 0);
  mesh.node_cap = n_nodes; mesh.prim_cap = n_prims; mesh.vert_cap = n_verts;
  mesh.bytes = blob.bytes.size();
  return HK_OK;
}

// ------------------------------------------------------------------ one-level BVH (DScene::flat, hk_device.hpp traverse_flat)
// Built on the host at every instance-level rebuild of a scene whose instances all share one transform and that fits the LDS
// copy: every triangle of every instance (local space = the one space they share), a top-down SAH build with an exact sweep
// along the three axes (the scenes are a few hundred triangles at most), one triangle per leaf, flattened depth-first with
// skip links once per ray-direction octant - each inner node's children in the order a ray of that octant meets them (axis
// of the larger centre separation), so a closest-hit walk finds its hit early and skips the rest by their boxes.
namespace flatbvh {
struct Tri { float lo[3], hi[3], c[3]; uint32_t prim, inst; };
struct Node { float lo[3], hi[3]; int left = -1, right = -1; uint32_t prim = 0, inst = 0; };
inline float half_area(const float* lo, const float* hi) {
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return dx * dy + dy * dz + dz * dx;
}
int build(std::vector<Node>& nodes, std::vector<Tri>& t, int b, int e) {
  const int id = (int)nodes.size();
  nodes.emplace_back();
  {
    Node& n = nodes[id];
    for (int k = 0; k < 3; ++k) { n.lo[k] = t[b].lo[k]; n.hi[k] = t[b].hi[k]; }
    for (int i = b + 1; i < e; ++i)
      for (int k = 0; k < 3; ++k) { n.lo[k] = std::min(n.lo[k], t[i].lo[k]); n.hi[k] = std::max(n.hi[k], t[i].hi[k]); }
  }
  if (e - b == 1) {
    nodes[id].prim = t[b].prim;
    nodes[id].inst = t[b].inst;
    return id;
  }
  const int n = e - b;
  double best = 1e300;
  int best_axis = 0, best_split = n / 2;
  std::vector<float> right_area((size_t)n);
  for (int axis = 0; axis < 3; ++axis) {
    std::stable_sort(t.begin() + b, t.begin() + e, [axis](const Tri& x, const Tri& y) { return x.c[axis] < y.c[axis]; });
    float lo[3], hi[3];
    for (int i = n - 1; i >= 1; --i) {  // right_area[i] = area of the box of t[b + i .. e)
      const Tri& q = t[b + i];
      for (int k = 0; k < 3; ++k) {
        lo[k] = i == n - 1 ? q.lo[k] : std::min(lo[k], q.lo[k]);
        hi[k] = i == n - 1 ? q.hi[k] : std::max(hi[k], q.hi[k]);
      }
      right_area[(size_t)i] = half_area(lo, hi);
    }
    for (int i = 1; i < n; ++i) {  // split: [b, b + i) | [b + i, e)
      const Tri& q = t[b + i - 1];
      for (int k = 0; k < 3; ++k) {
        lo[k] = i == 1 ? q.lo[k] : std::min(lo[k], q.lo[k]);
        hi[k] = i == 1 ? q.hi[k] : std::max(hi[k], q.hi[k]);
      }
      const double cost = (double)half_area(lo, hi) * i + (double)right_area[(size_t)i] * (n - i);
      if (cost < best) { best = cost; best_axis = axis; best_split = i; }
    }
  }
  std::stable_sort(t.begin() + b, t.begin() + e, [best_axis](const Tri& x, const Tri& y) { return x.c[best_axis] < y.c[best_axis]; });
  const int l = build(nodes, t, b, b + best_split);
  const int r = build(nodes, t, b + best_split, e);
  nodes[id].left = l;
  nodes[id].right = r;
  return id;
}
// depth-first flattening for direction octant `oct` (only the bits of `mask` are distinguished); returns the index after the subtree
uint32_t emit(const std::vector<Node>& nodes, int id, uint32_t oct, uint32_t mask, std::vector<float4>& out, uint32_t at) {
  const Node& n = nodes[id];
  if (n.left < 0) {
    out[2 * at] = make_float4(n.lo[0], n.lo[1], n.lo[2], as_f(HK_BVH_LEAF_FLAG | n.prim));
    out[2 * at + 1] = make_float4(n.hi[0], n.hi[1], n.hi[2], as_f((at + 1u) | (n.inst << 16)));
    return at + 1u;
  }
  const Node &a = nodes[n.left], &b = nodes[n.right];
  int axis = 0;
  float sep = -1.0f;
  for (int k = 0; k < 3; ++k) {
    const float d = std::fabs((b.lo[k] + b.hi[k]) - (a.lo[k] + a.hi[k]));
    if (d > sep) { sep = d; axis = k; }
  }
  const bool a_smaller = (a.lo[axis] + a.hi[axis]) <= (b.lo[axis] + b.hi[axis]);
  const bool negative = ((oct & mask) >> axis) & 1u;           // the ray travels towards smaller coordinates on this axis
  const bool a_first = negative ? !a_smaller : a_smaller;
  uint32_t next = emit(nodes, a_first ? n.left : n.right, oct, mask, out, at + 1u);
  next = emit(nodes, a_first ? n.right : n.left, oct, mask, out, next);
  out[2 * at] = make_float4(n.lo[0], n.lo[1], n.lo[2], as_f(at + 1u));
  out[2 * at + 1] = make_float4(n.hi[0], n.hi[1], n.hi[2], as_f(next));
  return next;
}
}  // namespace flatbvh

// Fills `out` with `orderings` flattenings of (2 T - 1) nodes each; returns false when the scene does not qualify.
bool build_flat_bvh(const hk_ctx* c, uint32_t orderings, std::vector<float4>& out, uint32_t& count) {
  using namespace flatbvh;
  std::vector<Tri> tris;
  for (size_t i = 0; i < c->instances.size(); ++i) {
    const HkInstance& in = c->instances[i];
    for (uint32_t k = 0; k < in.mesh.node_count; ++k) {
      const HkNode& nd = c->asset_nodes[in.mesh.node_offset + k];
      if (nd.entry_index < HK_BVH_LEAF_FLAG) continue;
      const size_t prim = (size_t)in.mesh.primitive + (nd.entry_index - HK_BVH_LEAF_FLAG);
      if (prim >= c->primitives.size() || prim > 0xFFFFu) return false;
      Tri t;
      const HkPrimitiveVertex* v = c->primitives[prim].vertices;
      for (int a = 0; a < 3; ++a) {
        t.lo[a] = hmin(v[0].position[a], hmin(v[1].position[a], v[2].position[a]));  // = the BLAS leaf box (light.wgsl:408-412)
        t.hi[a] = hmax(v[0].position[a], hmax(v[1].position[a], v[2].position[a]));
        t.c[a] = 0.5f * (t.lo[a] + t.hi[a]);
        if (!(t.lo[a] == t.lo[a]) || !(t.hi[a] == t.hi[a])) return false;  // NaN vertices: leave the scene to the reference walk
      }
      t.prim = (uint32_t)prim;
      t.inst = (uint32_t)i;
      tris.push_back(t);
    }
  }
  if (tris.empty() || tris.size() > 0x7FFFu) return false;
  std::vector<Node> nodes;
  nodes.reserve(2 * tris.size());
  build(nodes, tris, 0, (int)tris.size());
  count = (uint32_t)nodes.size();
  out.assign((size_t)orderings * count * 2, make_float4(0, 0, 0, 0));
  std::vector<float4> one((size_t)count * 2);
  for (uint32_t o = 0; o < orderings; ++o) {
    if (emit(nodes, 0, o, orderings - 1u, one, 0u) != count) return false;
    std::copy(one.begin(), one.end(), out.begin() + (size_t)o * count * 2);
  }
  return true;
}

int build_dynamic_region(hk_ctx* c, Blob& blob, DynOffsets& o, size_t mesh_bytes) {
  const size_t n_tlas = c->instance_nodes.size();
  const int orderings = c->threaded ? 8 : 1;
  std::vector<std::vector<HkNode>> ordered;
  // hk_update_scene_instances: the device is about to build every ordering of this tree in stream order - ordering 0 is laid
  // out (its leaf boxes are where the device build reads the instances' boxes from), the other seven slots stay zero
  const int host_orderings = c->trees_pending_on_device ? 1 : orderings;
  if (c->trees_pending_on_device) ordered.assign(1, c->instance_nodes);
  else thread_orderings(c->instance_nodes, {{0u, (uint32_t)n_tlas}}, orderings, ordered);
  std::vector<float4> tlo(n_tlas), thi(n_tlas);
  std::vector<float4>& tlas = c->tlas_tmp;
  tlas.clear();
  tlas.reserve(2 * n_tlas * (size_t)orderings);
  for (int ord = 0; ord < host_orderings; ++ord) {
    for (size_t i = 0; i < n_tlas; ++i) {
      const HkNode& n = ordered[ord][i];
      const float* mn = n.min;
      const float* mx = n.max;
      if (n.entry_index >= HK_BVH_LEAF_FLAG) {  // light.wgsl:454-457: the leaf box is the instance's world AABB
        uint32_t inst = n.entry_index - HK_BVH_LEAF_FLAG;
        HK_REQUIRE(inst < c->instances.size(), HK_E_INVALID, "TLAS leaf instance out of bounds");
        mn = c->instances[inst].min;
        mx = c->instances[inst].max;
      }
      tlo[i] = make_float4(mn[0], mn[1], mn[2], as_f(n.entry_index));
      thi[i] = make_float4(mx[0], mx[1], mx[2], as_f(n.exit_index));
    }
    fold_leaf_navigators(tlo, thi, 0, n_tlas);
    for (size_t i = 0; i < n_tlas; ++i) { tlas.push_back(tlo[i]); tlas.push_back(thi[i]); }
  }
  tlas.resize(2 * n_tlas * (size_t)orderings, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  o.tlas = blob.add(tlas);  // offset 0: ordering `ord` starts at node ord * n_tlas

  const bool have_prev = c->prev_models.size() == 16 * c->instances.size();
  std::vector<DInstance> di(c->instances.size());
  std::vector<float4> pm;
  bool any_moved = false;
  for (size_t i = 0; i < di.size(); ++i) {
    const HkInstance& in = c->instances[i];
    const float* t = in.inverse_transpose_model;
    const float* m = in.model;
    DInstance& d = di[i];
    d.im0 = make_float4(t[0], t[4], t[8], t[12]);  // column j of transpose(itm) = row j of itm
    d.im1 = make_float4(t[1], t[5], t[9], t[13]);
    d.im2 = make_float4(t[2], t[6], t[10], t[14]);
    d.im3 = make_float4(t[3], t[7], t[11], t[15]);
    d.m0 = make_float4(m[0], m[1], m[2], m[3]);
    d.m1 = make_float4(m[4], m[5], m[6], m[7]);
    d.m2 = make_float4(m[8], m[9], m[10], m[11]);
    d.m3 = make_float4(m[12], m[13], m[14], m[15]);
    d.n0 = make_float4(t[0], t[1], t[2], 0.0f);
    d.n1 = make_float4(t[4], t[5], t[6], 0.0f);
    d.n2 = make_float4(t[8], t[9], t[10], 0.0f);
    d.material = in.material;
    d.vertex = in.mesh.vertex;
    d.primitive = in.mesh.primitive;
    d.node_offset = in.mesh.node_offset;
    d.node_count = in.mesh.node_count;
    d.moved = (have_prev && memcmp(&c->prev_models[16 * i], m, 64) != 0) ? 1u : 0u;
    any_moved = any_moved || d.moved;
    d.pad1 = d.pad2 = 0;
  }
  if (any_moved) {  // previous model matrices, 4 columns per instance (only when something moves)
    pm.resize(4 * di.size());
    for (size_t i = 0; i < di.size(); ++i)
      for (int col = 0; col < 4; ++col) {
        const float* q = &c->prev_models[16 * i + 4 * col];
        pm[4 * i + col] = make_float4(q[0], q[1], q[2], q[3]);
      }
  }
  o.instances = blob.add(di);
  o.prev_models = blob.add(pm);

  const size_t n_light = c->emissive_nodes.size();
  std::vector<float4> llo(n_light), lhi(n_light);
  for (size_t i = 0; i < n_light; ++i) {
    const HkNode& n = c->emissive_nodes[i];
    float mn[3] = {n.min[0], n.min[1], n.min[2]}, mx[3] = {n.max[0], n.max[1], n.max[2]};
    if (n.entry_index >= HK_BVH_LEAF_FLAG) {  // light.wgsl:633-636: position -/+ radius
      uint32_t e = n.entry_index - HK_BVH_LEAF_FLAG;
      HK_REQUIRE(e < c->emissives.size(), HK_E_INVALID, "light BVH leaf out of bounds");
      for (int k = 0; k < 3; ++k) {
        mn[k] = c->emissives[e].position[k] - c->emissives[e].radius;
        mx[k] = c->emissives[e].position[k] + c->emissives[e].radius;
      }
    }
    llo[i] = make_float4(mn[0], mn[1], mn[2], as_f(n.entry_index));
    lhi[i] = make_float4(mx[0], mx[1], mx[2], as_f(n.exit_index));
  }
  fold_leaf_navigators(llo, lhi, 0, n_light);
  o.light_lo = blob.add(llo);
  o.light_hi = blob.add(lhi);

  std::vector<DEmissive> de(c->emissives.size());
  for (size_t i = 0; i < de.size(); ++i) {
    const HkEmissive& e = c->emissives[i];
    HK_REQUIRE(e.instance < c->instances.size(), HK_E_INVALID, "emissive instance out of bounds");
    HK_REQUIRE((size_t)e.alias_table[0] + e.alias_table[1] <= c->alias_table.size() && e.alias_table[1] > 0, HK_E_INVALID, "emissive alias slice out of bounds");
    de[i].position_radius = make_float4(e.position[0], e.position[1], e.position[2], e.radius);
    de[i].instance = e.instance;
    de[i].alias_offset = e.alias_table[0];
    de[i].alias_count = e.alias_table[1];
    de[i].surface_area = e.surface_area;
  }
  o.emissives = blob.add(de);
  std::vector<float2> al(c->alias_table.size());
  for (size_t i = 0; i < al.size(); ++i) al[i] = make_float2(c->alias_table[i].prob, as_f(c->alias_table[i].index));
  o.alias = blob.add(al);

  const uint32_t n_tex = (uint32_t)c->textures.size();
  std::vector<float4> mats(4 * c->materials.size());
  for (size_t i = 0; i < c->materials.size(); ++i) {
    const HkMaterial& m = c->materials[i];
    const uint32_t ids[4] = {m.base_color_texture, m.emissive_texture, m.metallic_roughness_texture, m.occlusion_texture};
    for (uint32_t id : ids)  // MaterialTextures::id, material.rs:76-86: an index into the texture array or u32::MAX
      HK_REQUIRE(id == HK_NO_TEXTURE || id < n_tex, HK_E_INVALID, "material %zu references texture %u but only %u textures are uploaded", i, id, n_tex);
    material_rows(m, &mats[4 * i]);
  }
  o.materials = blob.add(mats);
  // material textures: a 16-B descriptor per texture + the sRGB decode table (texels live in their own buffer)
  std::vector<uint4> tex_info(n_tex);
  size_t texel_offset = 0;
  for (uint32_t i = 0; i < n_tex; ++i) {
    const hk_ctx::HostTexture& t = c->textures[i];
    tex_info[i] = make_uint4((uint32_t)texel_offset, t.w, t.h, t.flags);
    texel_offset += t.texels.size();
  }
  std::vector<float> srgb_lut(256);
  srgb_decode_table(srgb_lut.data());  // (host_logic.cpp: the table hk_encode_texels inverts)
  o.tex_info = blob.add(tex_info);
  o.srgb_lut = blob.add(srgb_lut);
  blob.bytes.resize((blob.bytes.size() + 31) & ~(size_t)31, 0);
  // the one-level BVH (traverse_flat): only for scenes that stay inside the LDS copy WITH it, whose instances share one
  // transform, outside the bit-exact verification mode; as many direction orderings (8, 4, 2, 1) as fit
  o.flat = 0;
  o.flat_count = o.flat_orderings = 0;
  if (!(c->flags & HK_CTX_EXACT_TRAVERSAL) && !c->threaded && !c->instances.empty() && c->instances.size() <= 0xFFFFu && c->flat_walk) {
    bool shared = true;
    for (const HkInstance& in : c->instances)
      if (memcmp(in.inverse_transpose_model, c->instances[0].inverse_transpose_model, 64) != 0) shared = false;
    // direction orderings: as many (8, 4, 2, 1) as keep the node array within 4 KB - every workgroup copies the blob into LDS and
    // the LDS a workgroup holds bounds the workgroups per CU; measured on the Cornell box (71 nodes, tools/ab_flat.sh): 1 / 2 / 4 / 8
    // orderings walk equally fast (0.27 ms k_indirect) and the direct-light kernels lose 13 % with the 18 KB of eight
    uint32_t want = 8, budget = 4096;
    if (c->flat_orderings > 0) { want = (uint32_t)c->flat_orderings; budget = HK_LDS_SCENE_BYTES; }  // (hk_debug_set_option: the A/B of the orderings)
    while (want & (want - 1)) want &= want - 1;  // a power of two
    std::vector<float4> flat;
    uint32_t count = 0;
    if (shared && build_flat_bvh(c, 1u, flat, count)) {  // (a first build tells the node count: 2 T - 1)
      const size_t per_ordering = flat.size() * 16;
      uint32_t ord = want;
      while (ord > 1 && (per_ordering * ord > budget || blob.bytes.size() + per_ordering * ord + mesh_bytes > HK_LDS_SCENE_BYTES)) ord >>= 1;
      if (ord > 1 && !build_flat_bvh(c, ord, flat, count)) ord = 0;
      if (ord >= 1 && blob.bytes.size() + flat.size() * 16 + mesh_bytes <= HK_LDS_SCENE_BYTES && count <= 0xFFFFu) {
        o.flat = blob.add(flat);
        o.flat_count = count;
        o.flat_orderings = ord;
        blob.bytes.resize((blob.bytes.size() + 31) & ~(size_t)31, 0);
      }
    }
  }
  return HK_OK;
}

int join_side(hk_ctx* c);
int join_post(hk_ctx* c);
int join_all(hk_ctx* c);
// wait for everything the context has enqueued, on ALL streams (the direct-light dispatches of a frame may still be
// running on the side stream when a host uploads, resizes or reads statistics between two stages)
int sync_all(hk_ctx* c) {
  const int rc = join_all(c);
  if (rc) return rc;
  HK_HIP(hipStreamSynchronize(c->stream));
  poll_retired(c, false);  // (allocations an hk_add_meshes replaced: freed where the host has waited anyway)
  return HK_OK;
}

// DScene::shared_xform: every instance has the same inverse model (bit for bit), so a traversal transforms its ray once instead of
// once per instance entry (hk_device.hpp traverse_top).  Derived from the host mirrors: whoever changes an instance's pose - an
// upload or a device refit - has to call this before the next frame is enqueued.
void update_shared_transform(hk_ctx* c) {
  c->scene.shared_xform = 1u;
  for (const HkInstance& in : c->instances)
    if (memcmp(in.inverse_transpose_model, c->instances[0].inverse_transpose_model, 64) != 0) c->scene.shared_xform = 0u;
  // the one-level BVH lives in the shared LOCAL space: it stays valid while the instances move together and is simply not
  // walked once one of them moves on its own
  c->scene.flat_mode = (c->dyn_off.flat_count && c->scene.shared_xform) ? 1u : 0u;
  // ... nor once a mesh deformed on the device: the tree was built over the host's triangles (hikari_hip.h hk_update_mesh_vertices)
  if (c->meshes_deformed) c->scene.flat_mode = 0u;
  // ... and poses set from device memory are not in the mirrors this was derived from (hk_set_instance_transforms_device): neither shortcut
  if (c->poses_on_device) c->scene.shared_xform = c->scene.flat_mode = 0u;
}

// point c->scene at the arrays of the slot in use
void point_scene_at_slot(hk_ctx* c) {
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  const DynOffsets& o = c->dyn_off;
  const uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  const uint8_t* sbase = c->scene_mem + slots;
  DScene& s = c->scene;
  s.blob = (const float4*)base;  // (two slots: the scene is too big for the LDS copy, blob is not read)
  s.blob_f4 = (uint32_t)((slots + c->mesh.bytes) / 16);
  s.nodes = (const float4*)base;
  s.blas_base = (uint32_t)(((size_t)(sbase - base) + c->mesh.nodes) / 32);
  s.instances = (const DInstance*)(base + o.instances);
  c->d_prev_models = (const float4*)(base + o.prev_models);
  s.tri_v0 = (const float4*)(sbase + c->mesh.v0); s.tri_v1 = (const float4*)(sbase + c->mesh.v1); s.tri_v2 = (const float4*)(sbase + c->mesh.v2);
  s.vtx_normal = (const float4*)(sbase + c->mesh.vn); s.vtx_uv = (const float2*)(sbase + c->mesh.vuv);
  s.materials = (const float4*)(base + o.materials);
  s.tex_info = (const uint4*)(base + o.tex_info);
  s.srgb_lut = (const float*)(base + o.srgb_lut);
  s.tex_data = c->d_tex_data.p;
  s.n_textures = (uint32_t)c->textures.size();
  s.light_lo = (const float4*)(base + o.light_lo); s.light_hi = (const float4*)(base + o.light_hi);
  s.emissives = (const DEmissive*)(base + o.emissives); s.alias = (const float2*)(base + o.alias);
  s.noise = c->d_noise.p;
  s.tlas_count = (uint32_t)c->instance_nodes.size();
  s.tlas_stride = c->threaded ? (uint32_t)c->instance_nodes.size() : 0u;
  s.blas_stride = c->threaded ? (uint32_t)c->mesh.node_cap : 0u;  // (the capacity: hk_add_meshes leaves room behind the last tree)
  s.light_count = (uint32_t)c->emissive_nodes.size();
  s.flat = (const float4*)(base + o.flat);
  s.flat_count = o.flat_count;
  s.flat_mask = o.flat_orderings ? o.flat_orderings - 1u : 0u;
  update_shared_transform(c);
}
void repoint_scene(hk_ctx* c) {
  const float4* prev = c->d_prev_models;
  point_scene_at_slot(c);
  if (prev == c->rf_prev_models) c->d_prev_models = prev;  // (the refit's own plane is not part of the slot)
}

bool wants_threaded(const hk_ctx* c, size_t n_nodes, size_t n_prims, size_t n_verts) {
  const size_t est = n_nodes * 32 + n_prims * 48 + n_verts * 24 + c->instance_nodes.size() * 32 + c->instances.size() * 208 + c->materials.size() * 64 +
                     c->emissive_nodes.size() * 32 + c->alias_table.size() * 8;
  return !(c->flags & HK_CTX_EXACT_TRAVERSAL) && est > HK_LDS_SCENE_BYTES;
}
// (with the capacities equal to the sizes this is the layout build_static_region's blob has)
MeshRegion mesh_region_layout(const MeshSizes& caps, uint32_t orderings) {
  MeshRegion r{caps.nodes, caps.prims, caps.verts};
  r.v0 = caps.nodes * orderings * 32;  // (nodes at offset 0)
  r.v1 = r.v0 + caps.prims * 16;
  r.v2 = r.v1 + caps.prims * 16;
  r.vn = r.v2 + caps.prims * 16;
  r.vuv = r.vn + caps.verts * 16;
  r.bytes = (r.vuv + caps.verts * 8 + 15) & ~(size_t)15;
  return r;
}

// The instance-level region as last laid out (c->dyn_blob) into the slot in use - the one frames in flight do NOT read - of a two-slot
// scene, through pinned staging in stream order: neither the host nor the GPU waits (finalize_scene, hk_change_scene_instances)
int upload_slot_staged(hk_ctx* c) {
  uint8_t* const slot_mem = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  // (the slot written now was read by the frame before last: its direct-light dispatches may still sit on the side stream - round 6,
  // hk_context.hpp side_done - so the copy goes behind them)
  int rc;
  if ((rc = join_side(c))) return rc;
  const int k = c->slot;
  if (c->staging_pending[k]) {  // the copy that last read this staging buffer (two updates ago)
    HK_HIP(hipEventSynchronize(c->staging_done[k]));
    c->staging_pending[k] = false;
  }
  if (c->staging_bytes[k] < c->dyn_capacity) {
    if (c->staging[k]) (void)hipHostFree(c->staging[k]);
    c->staging[k] = nullptr;
    c->staging_bytes[k] = 0;
    HK_HIP(hipHostMalloc((void**)&c->staging[k], c->dyn_capacity, hipHostMallocDefault));
    c->staging_bytes[k] = c->dyn_capacity;
  }
  if (!c->staging_done[k]) HK_HIP(hipEventCreateWithFlags(&c->staging_done[k], hipEventDisableTiming));
  memcpy(c->staging[k], c->dyn_blob.bytes.data(), c->dyn_blob.bytes.size());
  memset(c->staging[k] + c->dyn_blob.bytes.size(), 0, c->dyn_capacity - c->dyn_blob.bytes.size());
  // a copy KERNEL reading the pinned buffer over PCIe: the update stays on the compute queue of the stream, between
  // the kernels of two frames, instead of a hand-off to an SDMA engine and back
  hipLaunchKernelGGL(k_copy_u4, dim3((unsigned)((c->dyn_capacity / 16 + 255) / 256)), dim3(256), 0, c->stream, (uint4*)slot_mem,
                     (const uint4*)c->staging[k], c->dyn_capacity / 16);
  HK_HIP(hipGetLastError());
  HK_HIP(hipEventRecord(c->staging_done[k], c->stream));
  c->staging_pending[k] = true;
  c->async_instance_uploads += 1;
  return HK_OK;
}

int finalize_scene(hk_ctx* c) {
  if (!c->mesh_dirty && !c->dynamic_dirty && !c->textures_dirty) return HK_OK;
  c->scene_epoch += 1;   // (scene memory is about to be written on the main stream: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "meshes, materials and instances must be uploaded first");
  const size_t n_nodes = c->asset_nodes.size();
  bool need_static = c->mesh_dirty || !c->scene_mem || c->node_prim_offset.size() != n_nodes;
  {  // direction-threaded flattenings for everything that will not be traversed from the LDS copy (an estimate of the blob size decides;
     // a scene near the limit that ends up outside LDS without them merely walks in the reference's order)
    const bool want = wants_threaded(c, n_nodes, c->primitives.size(), c->vertices.size());
    if (want != c->threaded) {
      c->threaded = want;
      need_static = true;
    }
  }
  for (const HkInstance& in : c->instances) {
    HK_REQUIRE((size_t)in.mesh.node_offset + in.mesh.node_count <= n_nodes, HK_E_INVALID, "instance mesh node range out of bounds");
    HK_REQUIRE(in.material < c->materials.size(), HK_E_INVALID, "instance material out of bounds");
    // a mesh range no earlier instance used: its leaf boxes have not been derived yet
    if (!need_static && in.mesh.node_count && (c->node_prim_offset[in.mesh.node_offset] != (int64_t)in.mesh.primitive ||
                                                c->node_prim_offset[in.mesh.node_offset + in.mesh.node_count - 1] != (int64_t)in.mesh.primitive))
      need_static = true;
  }
  int rc;
  if (c->textures_dirty) {
    std::vector<uint32_t> tex_data;
    for (const hk_ctx::HostTexture& t : c->textures) tex_data.insert(tex_data.end(), t.texels.begin(), t.texels.end());
    if ((rc = sync_all(c))) return rc;
    if ((rc = c->d_tex_data.upload(tex_data))) return rc;
    c->textures_dirty = false;
  }
  HK_REQUIRE(!(c->mirrors_stale && c->dynamic_dirty), HK_E_NOT_READY,
             "the instance-level arrays were last changed on the device (hk_refit_scene_instances): upload the instances again (hk_upload_scene_instances) "
             "before a change that rebuilds them on the host");
  HK_REQUIRE(!c->meshes_deformed, HK_E_NOT_READY,
             "a mesh was deformed on the device (hk_update_mesh_vertices / hk_skin_mesh): upload the host's mirror of it (hk_upload_scene) "
             "before a change that lays the scene out again on the host");
  Blob st;  // (the mesh-level region first: whether the one-level BVH still fits the LDS copy depends on its size)
  MeshRegion laid;
  if (need_static && (rc = build_static_region(c, st, laid))) return rc;
  Blob& dyn = c->dyn_blob;
  dyn.bytes.clear();
  DynOffsets o{};
  const double tb0_ = now_ms();
  if ((rc = build_dynamic_region(c, dyn, o, need_static ? laid.bytes : c->mesh.bytes))) return rc;
  if (c->trace_update) fprintf(stderr, "  build_dynamic_region %.2f ms (%zu bytes)\n", now_ms() - tb0_, dyn.bytes.size());
  c->dyn_off = o;
  c->rf_ready = false;
  c->rf_last_moved.clear();
  const bool in_place = !need_static && dyn.bytes.size() <= c->dyn_capacity;
  if (!(in_place && c->two_slots) && (rc = sync_all(c))) return rc;  // frames in flight still read the arrays rewritten below
  if (need_static) {
    if (c->scene_mem) { (void)hipFree(c->scene_mem); c->scene_mem = nullptr; }
    c->dyn_capacity = dyn.bytes.size();  // exact: a small scene stays small enough for the LDS copy
    c->mesh = laid;  // (a host layout is exact: no room to spare)
    c->two_slots = c->dyn_capacity + c->mesh.bytes > HK_LDS_SCENE_BYTES;
    c->slot = 0;
    // room for the previous model matrix of every instance, so that the first moving frame already fits its slot
    if (c->two_slots) c->dyn_capacity = (c->dyn_capacity + 64 * c->instances.size() + 31) & ~(size_t)31;
    const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
    HK_HIP(hipMalloc((void**)&c->scene_mem, slots + c->mesh.bytes));
    HK_HIP(hipMemcpy(c->scene_mem + slots, st.bytes.data(), st.bytes.size(), hipMemcpyHostToDevice));
  } else if (!in_place) {  // instance count grew: move the mesh region behind larger slots, device to device
    const size_t cap = ((dyn.bytes.size() + dyn.bytes.size() / 2) + 31) & ~(size_t)31;
    const size_t old_slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
    c->two_slots = c->two_slots || cap + c->mesh.bytes > HK_LDS_SCENE_BYTES;
    c->slot = 0;
    const size_t slots = (c->two_slots ? 2 : 1) * cap;
    uint8_t* mem = nullptr;
    HK_HIP(hipMalloc((void**)&mem, slots + c->mesh.bytes));
    HK_HIP(hipMemcpy(mem + slots, c->scene_mem + old_slots, c->mesh.bytes, hipMemcpyDeviceToDevice));
    (void)hipFree(c->scene_mem);
    c->scene_mem = mem;
    c->dyn_capacity = cap;
  } else if (c->two_slots) {
    c->slot ^= 1;
  }
  uint8_t* const slot_mem = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  if (in_place && c->two_slots) {
    if ((rc = upload_slot_staged(c))) return rc;
  } else {
    HK_HIP(hipMemcpy(slot_mem, dyn.bytes.data(), dyn.bytes.size(), hipMemcpyHostToDevice));
    if (dyn.bytes.size() < c->dyn_capacity) HK_HIP(hipMemset(slot_mem + dyn.bytes.size(), 0, c->dyn_capacity - dyn.bytes.size()));
  }

  point_scene_at_slot(c);
  c->mesh_dirty = c->dynamic_dirty = false;
  c->static_rebuilds += need_static ? 1 : 0;
  c->dynamic_rebuilds += 1;
  c->wide_tlas_dirty = true;                       // (the wide records follow the trees: context.hip ensure_wide)
  c->wide_mesh_check = true;                       // (... and the instance set may now use a mesh tree that has no records yet)
  if (need_static) c->wide_blas_dirty = true;
  return HK_OK;
}

}  // namespace hk

extern "C" {

int hk_upload_meshes(hk_ctx* c, const HkVertex* v, uint32_t nv, const HkPrimitive* p, uint32_t np, const HkNode* n, uint32_t nn) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && v && p && n && nv && np && nn, HK_E_INVALID, "NULL or empty mesh buffers");
  if (!c->deform.empty()) {  // (the trees and skins of the deformable meshes name the old topology; frames in flight may still use them)
    const int rc = sync_all(c);
    if (rc) return rc;
    free_deform(c);
  }
  c->meshes_deformed = false;
  c->vertices.assign(v, v + nv);
  c->primitives.assign(p, p + np);
  c->asset_nodes.assign(n, n + nn);
  c->have_meshes = true;
  c->mesh_dirty = true;
  return HK_OK;
}
int hk_upload_materials(hk_ctx* c, const HkMaterial* m, uint32_t n) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && m && n, HK_E_INVALID, "NULL or empty material buffer");
  c->materials.assign(m, m + n);
  c->have_materials = true;
  c->dynamic_dirty = true;
  return HK_OK;
}
int hk_upload_instances(hk_ctx* c, const HkInstance* inst, uint32_t ni, const HkNode* inodes, uint32_t nin, const HkEmissive* em, uint32_t ne,
                        const HkNode* enodes, uint32_t nen, const HkAliasEntry* alias, uint32_t na) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && inst && inodes && ni && nin, HK_E_INVALID, "NULL or empty instance buffers");
  HK_REQUIRE((em || !ne) && (enodes || !nen) && (alias || !na), HK_E_INVALID, "NULL emissive buffers");
  HK_REQUIRE(!c->meshes_deformed, HK_E_NOT_READY, "a mesh was deformed on the device: upload the host's mirror of it (hk_upload_scene) first");
  c->instances.assign(inst, inst + ni);
  c->instance_nodes.assign(inodes, inodes + nin);
  c->emissives.assign(em, em + ne);
  c->emissive_nodes.assign(enodes, enodes + nen);
  c->alias_table.assign(alias, alias + na);
  c->prev_models.clear();
  c->instances_generation += 1;
  c->have_instances = true;
  c->dynamic_dirty = true;
  c->mirrors_stale = false;
  c->poses_on_device = false;   // (the mirrors are the scene again: hk_set_instance_transforms_device)
  return HK_OK;
}
int hk_upload_previous_transforms(hk_ctx* c, const float* models, uint32_t n) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && (models || !n), HK_E_INVALID, "NULL argument");
  HK_REQUIRE(c->have_instances && n == c->instances.size(), HK_E_INVALID, "previous transforms must match the %zu uploaded instances", c->instances.size());
  c->prev_models.assign(models, models + 16 * (size_t)n);
  c->dynamic_dirty = true;
  return HK_OK;
}
#define HK_NO_STANDINS(b)                                                                                                        \
  HK_REQUIRE(!builder_has_standin_trees(b), HK_E_NOT_READY,                                                                      \
             "the builder holds stand-in trees (hk_scene_builder_finish_instances): finish it with hk_scene_builder_finish, or use " \
             "hk_update_scene_instances, which builds the trees on the device")
int hk_upload_scene(hk_ctx* c, const hk_scene_builder* b) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_NO_STANDINS(b);  // (frames from stand-in trees would differ silently in tie-breaks and visit order)
  HK_NO_UNRESOLVED_MESHES(b);
  HK_NO_PENDING_MESHES(b);
  return hk::upload_scene_unchecked(c, b);
}
}  // extern "C"
int hk::upload_scene_unchecked(hk_ctx* c, const hk_scene_builder* b) {
  const HkVertex* v; const HkPrimitive* p; const HkNode *an, *in_, *en; const HkMaterial* m; const HkInstance* inst; const HkEmissive* em; const HkAliasEntry* al;
  uint32_t nv, np, nan_, nm, ni, nin, ne, nen, nal;
  int rc;
  if ((rc = hk_scene_builder_vertices(b, &v, &nv))) return rc;
  if ((rc = hk_scene_builder_primitives(b, &p, &np))) return rc;
  if ((rc = hk_scene_builder_asset_nodes(b, &an, &nan_))) return rc;
  if ((rc = hk_scene_builder_materials(b, &m, &nm))) return rc;
  if ((rc = hk_scene_builder_instances(b, &inst, &ni))) return rc;
  if ((rc = hk_scene_builder_instance_nodes(b, &in_, &nin))) return rc;
  if ((rc = hk_scene_builder_emissives(b, &em, &ne))) return rc;
  if ((rc = hk_scene_builder_emissive_nodes(b, &en, &nen))) return rc;
  if ((rc = hk_scene_builder_alias_table(b, &al, &nal))) return rc;
  if ((rc = hk_upload_meshes(c, v, nv, p, np, an, nan_))) return rc;
  if ((rc = hk_upload_materials(c, m, nm))) return rc;
  if ((rc = hk_upload_instances(c, inst, ni, in_, nin, em, ne, en, nen, al, nal))) return rc;
  const float* pm; uint32_t npm;
  if ((rc = hk_scene_builder_previous_transforms(b, &pm, &npm))) return rc;
  return hk_upload_previous_transforms(c, pm, npm);
}
extern "C" {
int hk_upload_scene_instances(hk_ctx* c, const hk_scene_builder* b) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_NO_STANDINS(b);
  HK_NO_PENDING_MESHES(b);
  return hk::upload_scene_instances_unchecked(c, b);
}
}  // extern "C"
int hk::upload_scene_instances_unchecked(hk_ctx* c, const hk_scene_builder* b) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(c->have_meshes && c->have_materials, HK_E_NOT_READY, "hk_upload_scene must come first");
  const HkNode *in_, *en; const HkInstance* inst; const HkEmissive* em; const HkAliasEntry* al; const float* pm;
  uint32_t ni, nin, ne, nen, nal, npm;
  int rc;
  if ((rc = hk_scene_builder_instances(b, &inst, &ni))) return rc;
  if ((rc = hk_scene_builder_instance_nodes(b, &in_, &nin))) return rc;
  if ((rc = hk_scene_builder_emissives(b, &em, &ne))) return rc;
  if ((rc = hk_scene_builder_emissive_nodes(b, &en, &nen))) return rc;
  if ((rc = hk_scene_builder_alias_table(b, &al, &nal))) return rc;
  if ((rc = hk_scene_builder_previous_transforms(b, &pm, &npm))) return rc;
  if ((rc = hk_upload_instances(c, inst, ni, in_, nin, em, ne, en, nen, al, nal))) return rc;
  return hk_upload_previous_transforms(c, pm, npm);
}
extern "C" {
int hk_upload_textures(hk_ctx* c, const HkImageDesc* images, uint32_t n) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && (images || !n), HK_E_INVALID, "NULL argument");
  std::vector<hk_ctx::HostTexture> tex(n);
  for (uint32_t i = 0; i < n; ++i) {
    const HkImageDesc& d = images[i];
    HK_REQUIRE(d.rgba8 && d.width && d.height && d.width <= 16384 && d.height <= 16384, HK_E_INVALID, "image %u: bad pointer or size", i);
    HK_REQUIRE(d.address_u <= HK_ADDRESS_MIRROR_REPEAT && d.address_v <= HK_ADDRESS_MIRROR_REPEAT, HK_E_INVALID, "image %u: bad address mode", i);
    tex[i].w = d.width;
    tex[i].h = d.height;
    tex[i].flags = (d.is_srgb ? 1u : 0u) | (d.filter_linear ? 2u : 0u) | (d.address_u << 4) | (d.address_v << 6);
    tex[i].texels.resize((size_t)d.width * d.height);
    memcpy(tex[i].texels.data(), d.rgba8, tex[i].texels.size() * 4);
  }
  c->textures.swap(tex);
  c->tx_host_stale.clear();   // (every host copy is the scene again: hk_update_textures_device)
  c->textures_dirty = true;
  c->dynamic_dirty = true;
  return HK_OK;
}
// One texture's texels and sampler, in place (hikari_hip.h).  The texel buffer has ONE copy, like the mesh-level region: the write goes
// behind every frame enqueued so far on every stream that reads texels (stream waits through the context's events, no host wait).
int hk_update_texture(hk_ctx* c, uint32_t index, const HkImageDesc* image) {
  HK_REQUIRE(c && image && image->rgba8, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(!c->textures.empty(), HK_E_NOT_READY, "hk_upload_textures must come first");
  HK_REQUIRE(index < c->textures.size(), HK_E_INVALID, "texture %u of %zu", index, c->textures.size());
  hk_ctx::HostTexture& t = c->textures[index];
  HK_REQUIRE(image->width == t.w && image->height == t.h, HK_E_INVALID, "texture %u is %u x %u, the image %u x %u: a texture that changes size goes through hk_upload_textures",
             index, t.w, t.h, image->width, image->height);
  HK_REQUIRE(image->address_u <= HK_ADDRESS_MIRROR_REPEAT && image->address_v <= HK_ADDRESS_MIRROR_REPEAT, HK_E_INVALID, "bad address mode");
  c->scene_epoch += 1;   // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining - a refusal above leaves it alone)
  const uint32_t flags = (image->is_srgb ? 1u : 0u) | (image->filter_linear ? 2u : 0u) | (image->address_u << 4) | (image->address_v << 6);
  const size_t n = t.texels.size();
  size_t texel_offset = 0;
  for (uint32_t i = 0; i < index; ++i) texel_offset += c->textures[i].texels.size();
  // what a pending relayout (finalize_scene) is about to send anyway travels with it, from the mirror below
  const bool texels_live = !c->textures_dirty && c->d_tex_data.p && c->d_tex_data.n >= texel_offset + n;
  const bool info_live = !c->dynamic_dirty && !c->mesh_dirty && c->scene_mem;
  if (texels_live || info_live) {
    HK_HIP(hipSetDevice(c->device));
    int rc, k = 0;
    uint8_t* st = nullptr;
    if (texels_live) {
      if ((rc = stage(c, n * 4, &st, &k))) return rc;
      memcpy(st, image->rgba8, n * 4);
    }
    if ((rc = join_all(c))) return rc;
    uint4 *info0 = nullptr, *info1 = nullptr;
    if (info_live) {
      info0 = (uint4*)(c->scene_mem + c->dyn_off.tex_info) + index;
      if (c->two_slots) info1 = (uint4*)(c->scene_mem + c->dyn_capacity + c->dyn_off.tex_info) + index;
    }
    launch_texture_update(c->stream, c->d_tex_data.p + texel_offset, (const uint32_t*)st, texels_live ? n : 0, info0, info1, make_uint4((uint32_t)texel_offset, t.w, t.h, flags));
    HK_HIP(hipGetLastError());
    if (texels_live) {
      hk_ctx::DeformStage& s = c->df_stage[(size_t)k];
      HK_HIP(hipEventRecord(s.done, c->stream));
      s.pending = true;
    }
  }
  memcpy(t.texels.data(), image->rgba8, n * 4);
  t.flags = flags;
  if (index < c->tx_host_stale.size()) c->tx_host_stale[index] = 0;  // (the copy holds what the device does again)
  return HK_OK;
}
// Rectangles of many textures from the caller's DEVICE memory, converted in one launch (hikari_hip.h; kernels_scene.hip
// k_update_textures).  Ordered as hk_update_texture orders its write; only the item table and the workgroup table are staged.
int hk_update_textures_device(hk_ctx* c, const HkTextureSource* items, uint32_t n, void* producer_stream) {
  HK_REQUIRE(c && (items || !n), HK_E_INVALID, "NULL argument");
  HK_REQUIRE(!c->textures.empty(), HK_E_NOT_READY, "hk_upload_textures must come first");
  if (!n) return HK_OK;
  HK_HIP(hipSetDevice(c->device));
  int rc;
  // ---- the whole batch is validated before anything is enqueued or written
  const uint32_t n_tex = (uint32_t)c->textures.size();
  std::vector<uint32_t> new_flags(n_tex);
  for (uint32_t i = 0; i < n_tex; ++i) new_flags[i] = c->textures[i].flags;
  size_t n_blocks = 0;
  uint64_t texels = 0;
  bool any_encode = false;
  for (uint32_t i = 0; i < n; ++i) {
    const HkTextureSource& it = items[i];
    if ((rc = check_texture_source(it, i))) return rc;
    HK_REQUIRE(it.index < n_tex, HK_E_INVALID, "item %u: texture %u of %u", i, it.index, n_tex);
    const hk_ctx::HostTexture& t = c->textures[it.index];
    HK_REQUIRE((uint64_t)it.x0 + it.width <= t.w && (uint64_t)it.y0 + it.height <= t.h, HK_E_INVALID,
               "item %u: the rectangle (%u, %u) + %u x %u leaves texture %u of %u x %u", i, it.x0, it.y0, it.width, it.height, it.index, t.w, t.h);
    if (it.flags & HK_TEXTURE_SET_SAMPLER) {
      HK_REQUIRE(it.address_u <= HK_ADDRESS_MIRROR_REPEAT && it.address_v <= HK_ADDRESS_MIRROR_REPEAT, HK_E_INVALID, "item %u: bad address mode", i);
      new_flags[it.index] = (it.is_srgb ? 1u : 0u) | (it.filter_linear ? 2u : 0u) | (it.address_u << 4) | (it.address_v << 6);  // (of several items of a texture the last one)
    }
    for (uint32_t k = 0; k < i; ++k)
      HK_REQUIRE(!texture_rectangles_overlap(items[k], it), HK_E_INVALID, "items %u and %u overlap in texture %u: one launch cannot order them", k, i, it.index);
    if ((rc = check_source(c, i, "texels", it.data, texel_element_bytes(it.format), texture_source_extent(it)))) return rc;
    const uint32_t rows = std::max(1u, 2048u / it.width);
    n_blocks += (it.height + rows - 1u) / rows;
    texels += (uint64_t)it.width * it.height;
    any_encode = any_encode || (it.flags & HK_TEXTURE_LINEAR_SOURCE);
  }
  // ---- a pending hk_upload_textures is laid out first, as the next frame would; then the texel buffer is the device's
  if (c->textures_dirty && (rc = finalize_scene(c))) return rc;
  std::vector<size_t> offset(n_tex + 1, 0);
  for (uint32_t i = 0; i < n_tex; ++i) offset[i + 1] = offset[i] + c->textures[i].texels.size();
  HK_REQUIRE(c->d_tex_data.p && c->d_tex_data.n >= offset[n_tex], HK_E_NOT_READY, "the texel buffer is not on the device");
  const bool info_live = !c->dynamic_dirty && !c->mesh_dirty && c->scene_mem;  // (else the pending relayout writes the descriptors from the flags below)
  if (any_encode && !c->tx_thresholds) {  // once per context
    float mid[256];
    srgb_encode_thresholds(mid);
    HK_HIP(hipMalloc((void**)&c->tx_thresholds, sizeof(mid)));
    if (hipMemcpy(c->tx_thresholds, mid, sizeof(mid), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(c->tx_thresholds);
      c->tx_thresholds = nullptr;
      HK_REQUIRE(false, HK_E_HIP, "copying the sRGB thresholds failed: %s", hipGetErrorString(hipGetLastError()));
    }
  }
  hipStream_t producer = (hipStream_t)producer_stream;
  if (producer)
    for (hipEvent_t* e : {&c->tx_src_ready, &c->tx_src_read})
      if (!*e) HK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  // ---- the staging block: item table | workgroup table
  const size_t table_bytes = (n * sizeof(TextureItem) + 255) & ~(size_t)255;
  uint8_t* st = nullptr;
  int k = 0;
  if ((rc = stage(c, table_bytes + n_blocks * sizeof(SegmentBlock), &st, &k))) return rc;
  TextureItem* table = (TextureItem*)st;
  SegmentBlock* blocks = (SegmentBlock*)(st + table_bytes);
  size_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const HkTextureSource& it = items[i];
    const hk_ctx::HostTexture& t = c->textures[it.index];
    const uint32_t elem = texel_element_bytes(it.format);
    TextureItem d{};
    d.src = (const uint8_t*)it.data;
    d.stride_x = it.stride_x; d.stride_y = it.stride_y; d.stride_c = it.stride_c;
    d.dst = (uint32_t)(offset[it.index] + (size_t)it.y0 * t.w + it.x0);
    d.pitch = t.w;
    d.width = it.width; d.height = it.height;
    d.format = it.format; d.channels = it.channels;
    const size_t vec = 4u * elem;
    if ((it.flags & HK_TEXTURE_LINEAR_SOURCE) && (new_flags[it.index] & 1u)) d.mode |= HK_TEXTURE_ITEM_ENCODE;
    if (it.channels == 4u && it.stride_c == elem && (uintptr_t)it.data % vec == 0 && it.stride_x % vec == 0 && it.stride_y % vec == 0) d.mode |= HK_TEXTURE_ITEM_PACKED;
    d.rows = std::max(1u, 2048u / it.width);
    d.index = it.index;
    d.info = make_uint4((uint32_t)offset[it.index], t.w, t.h, new_flags[it.index]);
    table[i] = d;
    for (uint32_t first = 0; first < it.height; first += d.rows) blocks[at++] = SegmentBlock{i, first};
  }
  // ---- enqueue: behind every frame enqueued so far on every stream that reads texels (stream waits, no host wait)
  if ((rc = join_all(c))) return rc;
  if (producer) {  // what the producer has enqueued on the sources so far comes first; it may write them again once the launch has read them
    HK_HIP(hipEventRecord(c->tx_src_ready, producer));
    HK_HIP(hipStreamWaitEvent(c->stream, c->tx_src_ready, 0));
  }
  c->scene_epoch += 1;   // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining - a refusal above leaves it alone)
  uint4 *info0 = nullptr, *info1 = nullptr;
  if (info_live) {
    info0 = (uint4*)(c->scene_mem + c->dyn_off.tex_info);
    if (c->two_slots) info1 = (uint4*)(c->scene_mem + c->dyn_capacity + c->dyn_off.tex_info);
  }
  const uint32_t launches = launch_textures_update(c->stream, c->d_tex_data.p, table, blocks, (uint32_t)n_blocks, c->tx_thresholds, info0, info1,
                                                   producer ? c->tx_src_read : nullptr);
  HK_HIP(hipGetLastError());
  if (producer) HK_HIP(hipStreamWaitEvent(producer, c->tx_src_read, 0));
  hk_ctx::DeformStage& stg = c->df_stage[(size_t)k];
  HK_HIP(hipEventRecord(stg.done, c->stream));
  stg.pending = true;
  c->tx_host_stale.resize(n_tex, 0);
  for (uint32_t i = 0; i < n; ++i) c->tx_host_stale[items[i].index] = 1;
  for (uint32_t i = 0; i < n_tex; ++i) c->textures[i].flags = new_flags[i];
  c->last_texture_update[0] = n;
  c->last_texture_update[1] = launches;
  c->last_texture_update[2] = (uint32_t)std::min<uint64_t>(texels, 0xFFFFFFFFull);
  return HK_OK;
}
// ... and the way back: the device's texels of one texture, behind a wait for the context's streams; the host copy follows
int hk_read_texture(hk_ctx* c, uint32_t index, uint8_t* rgba8, size_t bytes) {
  HK_REQUIRE(c && rgba8, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(!c->textures.empty(), HK_E_NOT_READY, "hk_upload_textures must come first");
  HK_REQUIRE(index < c->textures.size(), HK_E_INVALID, "texture %u of %zu", index, c->textures.size());
  hk_ctx::HostTexture& t = c->textures[index];
  HK_REQUIRE(bytes == t.texels.size() * 4, HK_E_INVALID, "texture %u holds %zu bytes (%u x %u x 4), not %zu", index, t.texels.size() * 4, t.w, t.h, bytes);
  if (!c->textures_dirty) {  // (a pending hk_upload_textures: the copy IS what the device is about to hold)
    size_t texel_offset = 0;
    for (uint32_t i = 0; i < index; ++i) texel_offset += c->textures[i].texels.size();
    HK_REQUIRE(c->d_tex_data.p && c->d_tex_data.n >= texel_offset + t.texels.size(), HK_E_NOT_READY, "the texel buffer is not on the device");
    HK_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = sync_all(c))) return rc;
    HK_HIP(hipMemcpy(t.texels.data(), c->d_tex_data.p + texel_offset, bytes, hipMemcpyDeviceToHost));
    if (index < c->tx_host_stale.size()) c->tx_host_stale[index] = 0;
  }
  memcpy(rgba8, t.texels.data(), bytes);
  return HK_OK;
}
int hk_debug_last_texture_update(hk_ctx* c, uint32_t out[3]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 3; ++k) out[k] = c->last_texture_update[k];
  return HK_OK;
}
int hk_upload_noise(hk_ctx* c, const uint8_t* rgba, size_t bytes) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && rgba && bytes == 16u * 64u * 64u * 4u, HK_E_INVALID, "noise must be 16 tiles of 64x64 RGBA8 (262144 bytes)");
  HK_HIP(hipSetDevice(c->device));
  std::vector<uint32_t> words(16u * 64u * 64u);
  memcpy(words.data(), rgba, bytes);
  int rc = c->d_noise.upload(words);
  if (rc) return rc;
  c->scene.noise = c->d_noise.p;
  c->have_noise = true;
  return HK_OK;
}
}  // extern "C"
