// scene_append.hip - meshes added to a loaded scene on the device (hikari_hip.h hk_add_meshes; kernels in kernels_scene.hip).
// The reference re-concatenates its three mesh buffers whenever a mesh asset arrives (mesh.rs:106-166).  Here the mesh-level region keeps
// CAPACITIES behind its sub-arrays: the new meshes' records go through pinned staging to the end of the planes, their trees are built
// into the end of every ordering's node plane (the forest build of hk_load_scene) or - trees the host built - laid out for their ranges
// alone, and nothing of the existing meshes or of the instance level is read or written.  When the room runs out the whole scene moves
// once, device to device in stream order, to an allocation half again as large (scene_move.hip); the old one is freed behind the frames in flight.
#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

namespace {
// The scene copied into the allocation of `m` in ONE launch - both instance-level slots where they keep their size, else the slot in use
// (the spare one is about to be written); of every plane what the mirrors hold - and the switch.  A failure leaves the scene the context had.
int copy_and_commit(hk_ctx* c, SceneMove* m) {
  const size_t held[3] = {c->asset_nodes.size(), c->primitives.size(), c->vertices.size()};
  CopySegments s;
  if (m->dyn_capacity == c->dyn_capacity) s.add(m->mem, c->scene_mem, 2 * c->dyn_capacity);
  else s.add(m->mem + (size_t)c->slot * m->dyn_capacity, c->scene_mem + (size_t)c->slot * c->dyn_capacity, c->dyn_capacity);
  MovePlane planes[HK_MOVE_PLANES];
  for (uint32_t k = 0, n = move_planes(c, *m, planes); k < n; ++k) s.add(planes[k].dst, planes[k].src, std::min(planes[k].old_cap, held[planes[k].list]) << planes[k].shift);
  if (!s.overflow) launch_copy_segments(c->stream, s);  // (more sub-arrays than the table holds: nothing is enqueued)
  if (s.overflow || hipGetLastError() != hipSuccess) {
    const hipError_t e = hipGetLastError();
    move_abort(c, m, true);  // (the copy may be enqueued)
    HK_REQUIRE(false, HK_E_HIP, "the move of the scene failed: %s", hipGetErrorString(e));
  }
  return move_commit(c, m, c->slot);
}

// final form of the trees the host built, for the node span [first, first + count) that holds them: every ordering threaded, leaf boxes
// filled in, single-leaf navigators folded (scene_layout.hip build_static_region, for these ranges only); out = orderings x count x 2 float4
int layout_host_trees(const hk_ctx* c, const std::vector<LoadMesh>& meshes, uint32_t first, uint32_t count, int orderings, float4* out) {
  std::vector<HkNode> src(c->asset_nodes.begin() + first, c->asset_nodes.begin() + first + count);
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  for (const LoadMesh& m : meshes) ranges.emplace_back(m.index.node_offset - first, m.index.node_count);
  std::vector<std::vector<HkNode>> ordered;
  thread_orderings(src, ranges, orderings, ordered);
  std::vector<float4> lo(count), hi(count);
  const size_t n_prims = c->primitives.size();
  for (int o = 0; o < orderings; ++o) {
    const std::vector<HkNode>& nodes = ordered[(size_t)o];
    for (uint32_t i = 0; i < count; ++i) {
      lo[i] = make_float4(nodes[i].min[0], nodes[i].min[1], nodes[i].min[2], as_f(nodes[i].entry_index));
      hi[i] = make_float4(nodes[i].max[0], nodes[i].max[1], nodes[i].max[2], as_f(nodes[i].exit_index));
    }
    for (const LoadMesh& m : meshes) {
      const uint32_t base = m.index.node_offset - first;
      for (uint32_t k = 0; k < m.index.node_count; ++k) {
        const HkNode& n = nodes[base + k];
        if (n.entry_index < HK_BVH_LEAF_FLAG) continue;  // light.wgsl:408-412
        const size_t prim = (size_t)m.index.primitive + (n.entry_index - HK_BVH_LEAF_FLAG);
        HK_REQUIRE(prim < n_prims, HK_E_INVALID, "BLAS leaf primitive out of bounds");
        const HkPrimitiveVertex* v = c->primitives[prim].vertices;
        float mn[3], mx[3];
        for (int a = 0; a < 3; ++a) {
          mn[a] = hmin(v[0].position[a], hmin(v[1].position[a], v[2].position[a]));
          mx[a] = hmax(v[0].position[a], hmax(v[1].position[a], v[2].position[a]));
        }
        lo[base + k] = make_float4(mn[0], mn[1], mn[2], as_f(n.entry_index));
        hi[base + k] = make_float4(mx[0], mx[1], mx[2], as_f(n.exit_index));
      }
      fold_leaf_navigators(lo, hi, base, m.index.node_count);
    }
    float4* plane = out + 2 * (size_t)o * count;
    for (uint32_t i = 0; i < count; ++i) { plane[2 * i] = lo[i]; plane[2 * i + 1] = hi[i]; }
  }
  return HK_OK;
}

}  // namespace
// hk_change_scene_instances: the same move for larger instance-level slots, the mesh level keeping its capacities
int hk::grow_instance_slots(hk_ctx* c, size_t dyn_capacity) {
  SceneMove m;
  const int rc = move_begin(c, MeshSizes{c->mesh.node_cap, c->mesh.prim_cap, c->mesh.vert_cap}, dyn_capacity, c->wide_blas, c->wide_blas_rank, 0, "no room for the grown scene", &m);
  return rc ? rc : copy_and_commit(c, &m);
}
namespace {

// hk_debug_last_add / hk_debug_last_add_times start from zero once a call can no longer be refused
void clear_add_report(hk_ctx* c) {
  for (uint32_t& v : c->last_add) v = 0u;
  for (double& v : c->last_add_ms) v = 0.0;
}

// what hk_load_scene does for the whole builder: scenes walked from the LDS copy, and additions that change the ordering count
int full_layout(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode, uint32_t host_built) {
  HK_REQUIRE(!c->mirrors_stale && !c->meshes_deformed, HK_E_NOT_READY,
             "the scene was last changed on the device and this addition lays it out again on the host: upload the host's mirror first (hk_upload_scene)");
  clear_add_report(c);
  int rc = hk_load_scene(c, b, tree_mode);
  if (!rc) rc = finalize_scene(c);
  if (rc) return rc;
  c->last_add[0] = c->last_load[0];
  c->last_add[1] = c->last_load[1];
  c->last_add[2] = c->last_load[2];
  c->last_add[3] = host_built + c->last_load[3];
  return HK_OK;
}
}  // namespace

extern "C" {

int hk_add_meshes(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(tree_mode == HK_TREE_SAH || tree_mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", tree_mode);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene or hk_load_scene must come first");
  const HkVertex* bv = nullptr;
  const HkPrimitive* bp = nullptr;
  const HkNode* bn = nullptr;
  uint32_t nv = 0, np = 0, nn = 0;
  int rc;
  if ((rc = hk_scene_builder_vertices(b, &bv, &nv))) return rc;  // (HK_E_NOT_READY: not finished)
  if ((rc = hk_scene_builder_primitives(b, &bp, &np))) return rc;
  if ((rc = hk_scene_builder_asset_nodes(b, &bn, &nn))) return rc;
  HK_REQUIRE(!builder_has_standin_trees(b), HK_E_NOT_READY,
             "the builder holds stand-in instance trees (hk_scene_builder_finish_instances): finish it with hk_scene_builder_finish before hk_add_meshes");
  // ---- the builder's first meshes are the context's
  const MeshSizes old{c->asset_nodes.size(), c->primitives.size(), c->vertices.size()};
  const uint32_t n_meshes = builder_mesh_count(b);
  // (the builder concatenates in id order: the records are sorted, and a search finds a mesh without a copy of all of them)
  auto record = [b](uint32_t id) { HkMeshIndex m{}; (void)hk_scene_builder_mesh_index(b, id, &m); return m; };
  auto first_at = [&](uint32_t node_offset, uint32_t end) {  // the first of the meshes [0, end) whose nodes begin at or behind node_offset
    uint32_t lo = 0, hi = end;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (record(mid).node_offset < node_offset) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  {
    HkMeshIndex probe;
    if (n_meshes && (rc = hk_scene_builder_mesh_index(b, n_meshes - 1, &probe))) return rc;
  }
  HK_REQUIRE(old.nodes <= 0xFFFFFFFFull, HK_E_INVALID, "more mesh nodes than an HkMeshIndex can name");
  const uint32_t first_new = first_at((uint32_t)old.nodes, n_meshes);
  std::vector<HkMeshIndex> index(n_meshes);  // (filled for the new meshes only)
  for (uint32_t id = first_new; id < n_meshes; ++id) index[id] = record(id);
  {
    const HkMeshIndex end = first_new < n_meshes ? index[first_new] : HkMeshIndex{nv, np, nn, 0u};
    HK_REQUIRE(first_new > 0 && end.node_offset == old.nodes && end.primitive == old.prims && end.vertex == old.verts, HK_E_INVALID,
               "the builder's first meshes are not the context's: %zu nodes, %zu primitives and %zu vertices are uploaded, the builder's mesh %u begins at %u / %u / %u",
               old.nodes, old.prims, old.verts, first_new, end.node_offset, end.primitive, end.vertex);
    uint32_t new_pending = 0;
    for (uint32_t id = first_new; id < n_meshes; ++id) new_pending += builder_pending_mesh(b, id, nullptr) ? 1u : 0u;
    HK_REQUIRE(builder_pending_mesh_count(b) == new_pending, HK_E_INVALID, "a mesh among the builder's first %u is deferred, the context's meshes have their trees", first_new);
    for (const HkInstance& in : c->instances) {  // the records the instances carry are the builder's
      const uint32_t at = first_at(in.mesh.node_offset, first_new);
      const HkMeshIndex held = at < first_new ? record(at) : HkMeshIndex{};
      HK_REQUIRE(at < first_new && memcmp(&held, &in.mesh, sizeof(HkMeshIndex)) == 0, HK_E_INVALID,
                 "an uploaded instance carries the mesh record (%u, %u, %u, %u), which the builder does not hold", in.mesh.vertex, in.mesh.primitive, in.mesh.node_offset,
                 in.mesh.node_count);
    }
  }
  // (the report of the last add is cleared behind the last refusal - HK_E_NOT_READY, nothing written - as hk_remove_meshes clears its own)
  if (first_new == n_meshes) {  // nothing new: nothing is enqueued
    clear_add_report(c);
    return HK_OK;
  }
  HK_HIP(hipSetDevice(c->device));
  uint32_t n_host_built = 0;
  for (uint32_t id = first_new; id < n_meshes; ++id) n_host_built += builder_pending_mesh(b, id, nullptr) ? 0u : 1u;
  if (c->mesh_dirty || !c->scene_mem) return full_layout(c, b, tree_mode, n_host_built);  // (uploaded, not laid out yet)
  if ((rc = finalize_scene(c))) return rc;
  const MeshSizes now{nn, np, nv};
  if (!c->two_slots || wants_threaded(c, now.nodes, now.prims, now.verts) != c->threaded) return full_layout(c, b, tree_mode, n_host_built);
  clear_add_report(c);

  // ---- the device append.  Deferred meshes beyond the device limit are completed by the host's builder first
  std::vector<LoadMesh> device, host;
  for (uint32_t id = first_new; id < n_meshes; ++id) {
    LoadMesh m{id, index[id], 0u};
    HK_REQUIRE(m.index.node_count >= 1u && (m.index.node_count + 2u) % 3u == 0u, HK_E_INVALID, "mesh %u: a tree of %u nodes", id, m.index.node_count);
    m.n_tris = (m.index.node_count + 2u) / 3u;
    HK_REQUIRE((size_t)m.index.node_offset + m.index.node_count <= now.nodes && (size_t)m.index.primitive + m.n_tris <= now.prims && m.index.vertex <= now.verts, HK_E_INVALID,
               "the record of mesh %u lies outside the builder's mesh arrays", id);
    bool pending = builder_pending_mesh(b, id, nullptr);
    if (pending && m.n_tris > c->load_device_limit) {
      if ((rc = builder_complete_mesh_on_host(b, id))) return rc;
      pending = false;
    }
    (pending ? device : host).push_back(m);
  }
  const int orderings = c->threaded ? 8 : 1;
  if ((rc = join_all(c))) return rc;  // (the mesh-level region has one copy; a move goes behind every frame enqueued so far)
  uint32_t relocated = 0;
  if (now.nodes > c->mesh.node_cap || now.prims > c->mesh.prim_cap || now.verts > c->mesh.vert_cap) {  // (refused: nothing was written, the scene is the one it had)
    SceneMove m;
    const double t0 = now_ms();
    if ((rc = move_begin(c, move_room(now), c->dyn_capacity, c->wide_blas, c->wide_blas_rank, 0, "no room for the grown scene", &m))) return rc;
    const double t1 = now_ms();
    c->last_add_ms[0] = t1 - t0;
    if ((rc = copy_and_commit(c, &m))) return rc;
    c->last_add_ms[1] = now_ms() - t1;
    relocated = 1;
  }
  c->scene_epoch += 1;  // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining)
  // ---- from here on a failure leaves the context without a scene
  auto fail = [c](int code) {
    c->have_meshes = false;
    c->mesh_dirty = true;
    return code;
  };
  double t0 = now_ms();
  c->vertices.insert(c->vertices.end(), bv + old.verts, bv + now.verts);
  c->primitives.insert(c->primitives.end(), bp + old.prims, bp + now.prims);
  c->asset_nodes.insert(c->asset_nodes.end(), bn + old.nodes, bn + now.nodes);
  c->node_prim_offset.resize(now.nodes, -1);
  for (uint32_t id = first_new; id < n_meshes; ++id)  // final form whether an instance uses the range yet or not: a later instance finds it laid out
    std::fill(c->node_prim_offset.begin() + index[id].node_offset, c->node_prim_offset.begin() + index[id].node_offset + index[id].node_count, (int64_t)index[id].primitive);
  c->last_add_ms[2] = now_ms() - t0;
  t0 = now_ms();
  uint8_t* sbase = c->scene_mem + 2 * c->dyn_capacity;
  const uint32_t span = (uint32_t)(now.nodes - old.nodes), add_prims = (uint32_t)(now.prims - old.prims), add_verts = (uint32_t)(now.verts - old.verts);
  // the records as the builder holds them, and the laid-out span of the host-built trees, through one pinned buffer
  const size_t prim_bytes = (size_t)add_prims * sizeof(HkPrimitive), vert_bytes = (size_t)add_verts * sizeof(HkVertex);
  const size_t node_bytes = host.empty() ? 0 : (size_t)orderings * span * 32;
  static_assert(sizeof(HkPrimitive) == 48 && sizeof(HkVertex) == 32, "the append kernel reads 16-B pieces of these records");
  uint8_t* st = nullptr;
  int k = 0;
  if ((rc = stage(c, prim_bytes + vert_bytes + node_bytes + 16, &st, &k))) return fail(rc);
  memcpy(st, bp + old.prims, prim_bytes);
  memcpy(st + prim_bytes, bv + old.verts, vert_bytes);
  launch_append_geometry(c->stream, (const uint4*)st, add_prims, (const uint4*)(st + prim_bytes), add_verts, (float4*)(sbase + c->mesh.v0) + old.prims,
                         (float4*)(sbase + c->mesh.v1) + old.prims, (float4*)(sbase + c->mesh.v2) + old.prims, (float4*)(sbase + c->mesh.vn) + old.verts,
                         (float2*)(sbase + c->mesh.vuv) + old.verts);
  if (!host.empty()) {
    float4* laid = (float4*)(st + prim_bytes + vert_bytes);
    if ((rc = layout_host_trees(c, host, (uint32_t)old.nodes, span, orderings, laid))) return fail(rc);
    CopySegments s;  // (the deferred ranges of the span carry their stand-ins: the build below overwrites them in stream order)
    for (int o = 0; o < orderings; ++o) s.add(sbase + c->mesh.nodes + ((size_t)o * c->mesh.node_cap + old.nodes) * 32, laid + 2 * (size_t)o * span, (size_t)span * 32);
    if (s.overflow) {
      set_error("more orderings than one copy launch takes");
      return fail(HK_E_INVALID);
    }
    launch_copy_segments(c->stream, s);
  }
  hk_ctx::DeformStage& ds = c->df_stage[(size_t)k];
  if (hipGetLastError() != hipSuccess || hipEventRecord(ds.done, c->stream) != hipSuccess) {
    set_error("the append of the new meshes failed: %s", hipGetErrorString(hipGetLastError()));
    (void)hipStreamSynchronize(c->stream);
    return fail(HK_E_HIP);
  }
  ds.pending = true;
  uint32_t launches = 0;
  if (!device.empty() && (rc = build_on_device(c, b, device, tree_mode, &launches, false))) return fail(rc);  // (its one wait: on this call's own work)
  c->last_add_ms[3] = now_ms() - t0;
  c->device_tree_builds += device.size();
  c->last_add[0] = (uint32_t)device.size();
  for (const LoadMesh& m : device) c->last_add[1] += m.n_tris;
  c->last_add[2] = launches;
  c->last_add[3] = (uint32_t)host.size();
  c->last_add[4] = relocated;
  return HK_OK;
}

// Measurement hook (hikari_hip_debug.h): where the host time of the last hk_add_meshes went
int hk_debug_last_add_times(hk_ctx* c, double out[4]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = c->last_add_ms[k];
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): what the last hk_add_meshes did
int hk_debug_last_add(hk_ctx* c, uint32_t out[5]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 5; ++k) out[k] = c->last_add[k];
  return HK_OK;
}

}  // extern "C"
