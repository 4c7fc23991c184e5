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

namespace {
// What hk_add_meshes and hk_add_meshes_device share.  AddPlan: the builder's arrays and which of its meshes are new to the context.
// DeviceRecords: where the call's device block holds the records of the meshes that came from device memory.
struct AddPlan {
  const HkVertex* bv = nullptr;
  const HkPrimitive* bp = nullptr;
  const HkNode* bn = nullptr;
  uint32_t nv = 0, np = 0, nn = 0;
  MeshSizes old{0, 0, 0};
  uint32_t n_meshes = 0, first_new = 0;
  std::vector<HkMeshIndex> index;  // (filled for the new meshes only)
};
struct DeviceRecords {
  struct At { uint32_t mesh_id; const uint4 *prims, *verts; };
  std::vector<At> at;  // ascending mesh id; device memory
  const At* find(uint32_t id) const {
    for (const At& a : at)
      if (a.mesh_id == id) return &a;
    return nullptr;
  }
};

// every refusal of hk_add_meshes: nothing is written or enqueued
int add_check(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode, AddPlan* plan) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(tree_mode == HK_TREE_SAH || tree_mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", tree_mode);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene or hk_load_scene must come first");
  AddPlan& p = *plan;
  int rc;
  if ((rc = hk_scene_builder_vertices(b, &p.bv, &p.nv))) return rc;  // (HK_E_NOT_READY: not finished)
  if ((rc = hk_scene_builder_primitives(b, &p.bp, &p.np))) return rc;
  if ((rc = hk_scene_builder_asset_nodes(b, &p.bn, &p.nn))) return rc;
  const uint32_t nv = p.nv, np = p.np, nn = p.nn;
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
  std::vector<HkMeshIndex>& index = p.index;
  index.assign(n_meshes, HkMeshIndex{});
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
  p.old = old;
  p.n_meshes = n_meshes;
  p.first_new = first_new;
  return HK_OK;
}

// ... and what both do once nothing can be refused any more.  `dev` (or NULL): meshes whose records lie in device memory already - the
// append reads those from there, only the others are staged
int add_body(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode, const AddPlan& p, const DeviceRecords* dev) {
  const HkVertex* bv = p.bv;
  const HkPrimitive* bp = p.bp;
  const HkNode* bn = p.bn;
  const uint32_t nv = p.nv, np = p.np, nn = p.nn, n_meshes = p.n_meshes, first_new = p.first_new;
  const MeshSizes old = p.old;
  const std::vector<HkMeshIndex>& index = p.index;
  int rc;
  // (the report of the last add is cleared behind the last refusal - HK_E_NOT_READY, nothing written - as hk_remove_meshes clears its own)
  if (first_new == n_meshes) {  // nothing new: nothing is enqueued
    clear_add_report(c);
    return HK_OK;
  }
  HK_HIP(hipSetDevice(c->device));
  uint32_t n_host_built = 0;
  for (uint32_t id = first_new; id < n_meshes; ++id) n_host_built += builder_pending_mesh(b, id, nullptr) ? 0u : 1u;
  auto full = [&]() {  // (the builder is complete: the layout uploads the whole mesh level, whatever came from device memory)
    const int code = full_layout(c, b, tree_mode, n_host_built);
    if (!code) c->last_add_sources[3] = (uint32_t)std::min<size_t>((size_t)np * sizeof(HkPrimitive) + (size_t)nv * sizeof(HkVertex), 0xFFFFFFFFull);
    return code;
  };
  if (c->mesh_dirty || !c->scene_mem) return full();  // (uploaded, not laid out yet)
  if ((rc = finalize_scene(c))) return rc;
  const MeshSizes now{nn, np, nv};
  if (!c->two_slots || wants_threaded(c, now.nodes, now.prims, now.verts) != c->threaded) return full();
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
  const uint32_t span = (uint32_t)(now.nodes - old.nodes);
  // The new range as runs of consecutive meshes of one kind: those the host added - their records as the builder holds them, through one
  // pinned buffer with the laid-out span of the host-built trees - and those assembled from device memory, read where the block holds them
  // (consecutive sources lie consecutively there).  One append launch per run: one for a call of either kind alone.
  struct Run { bool device; uint32_t prim0, n_prims, vert0, n_verts; const uint4 *prims, *verts; };
  std::vector<Run> runs;
  size_t prim_bytes = 0, vert_bytes = 0;
  for (uint32_t id = first_new; id < n_meshes; ++id) {
    const DeviceRecords::At* at = dev ? dev->find(id) : nullptr;
    const uint32_t verts_end = id + 1u < n_meshes ? index[id + 1u].vertex : nv, n_tris = (index[id].node_count + 2u) / 3u;
    if (runs.empty() || runs.back().device != (at != nullptr)) runs.push_back(Run{at != nullptr, index[id].primitive, 0u, index[id].vertex, 0u, at ? at->prims : nullptr, at ? at->verts : nullptr});
    runs.back().n_prims += n_tris;
    runs.back().n_verts += verts_end - index[id].vertex;
    if (!at) {
      prim_bytes += (size_t)n_tris * sizeof(HkPrimitive);
      vert_bytes += (size_t)(verts_end - index[id].vertex) * sizeof(HkVertex);
    }
  }
  const size_t node_bytes = host.empty() ? 0 : (size_t)orderings * span * 32;
  static_assert(sizeof(HkPrimitive) == 48 && sizeof(HkVertex) == 32, "the append kernel reads 16-B pieces of these records");
  uint8_t* st = nullptr;
  int k = 0;
  if ((rc = stage(c, prim_bytes + vert_bytes + node_bytes + 16, &st, &k))) return fail(rc);
  {
    uint8_t *sp = st, *sv = st + prim_bytes;
    for (Run& r : runs) {
      if (!r.device) {
        memcpy(sp, bp + r.prim0, (size_t)r.n_prims * sizeof(HkPrimitive));
        memcpy(sv, bv + r.vert0, (size_t)r.n_verts * sizeof(HkVertex));
        r.prims = (const uint4*)sp;
        r.verts = (const uint4*)sv;
        sp += (size_t)r.n_prims * sizeof(HkPrimitive);
        sv += (size_t)r.n_verts * sizeof(HkVertex);
      }
      launch_append_geometry(c->stream, r.prims, r.n_prims, r.verts, r.n_verts, (float4*)(sbase + c->mesh.v0) + r.prim0, (float4*)(sbase + c->mesh.v1) + r.prim0,
                             (float4*)(sbase + c->mesh.v2) + r.prim0, (float4*)(sbase + c->mesh.vn) + r.vert0, (float2*)(sbase + c->mesh.vuv) + r.vert0);
    }
  }
  c->last_add_sources[3] = (uint32_t)std::min<size_t>(prim_bytes + vert_bytes, 0xFFFFFFFFull);
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
}  // namespace

extern "C" {

int hk_add_meshes(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_NO_UNRESOLVED_MESHES(b);  // (declared meshes hold zeros: hk_add_meshes_device or hk_scene_builder_resolve_mesh fills them)
  AddPlan plan;
  const int rc = add_check(c, b, tree_mode, &plan);
  if (rc) return rc;
  for (uint32_t& v : c->last_add_sources) v = 0u;
  for (double& v : c->last_add_source_ms) v = 0.0;
  return add_body(c, b, tree_mode, plan, nullptr);
}

// Meshes whose arrays lie in the caller's DEVICE memory (hikari_hip.h; kernels_scene.hip k_assemble_meshes; DESIGN 3 "Meshes from device
// memory").  Phase 0 validates the batch on the host; phase 1 assembles the reference records of every source in one launch into the
// context's device block and reads block and status back in one copy; phase 2 hands the records to the builder (the meshes are then what
// hk_scene_builder_add_mesh_deferred makes); phase 3 is hk_add_meshes' body, its append reading these meshes' records from the block.
int hk_add_meshes_device(hk_ctx* c, hk_scene_builder* b, const HkMeshSource* sources, uint32_t n, uint32_t tree_mode, void* producer_stream) {
  HK_REQUIRE(c && b && (sources || !n), HK_E_INVALID, "NULL argument");
  AddPlan plan;
  int rc;
  if ((rc = add_check(c, b, tree_mode, &plan))) return rc;
  // ---- phase 0: every unresolved mesh named by exactly one source, every pointer readable over its whole extent
  auto stride_of = [](uint32_t given, uint32_t packed) { return given ? given : packed; };
  std::vector<DeclaredMesh> decl(n);
  for (uint32_t i = 0; i < n; ++i) {
    const HkMeshSource& s = sources[i];
    HK_REQUIRE(s.flags == 0u, HK_E_INVALID, "source %u: unknown flags %#x", i, s.flags);
    HK_REQUIRE(s.mesh_id >= plan.first_new && builder_unresolved_mesh(b, s.mesh_id, &decl[i]), HK_E_INVALID,
               "source %u: mesh %u is not a declared mesh that waits for its arrays (hk_scene_builder_declare_mesh)", i, s.mesh_id);
    for (uint32_t k = 0; k < i; ++k) HK_REQUIRE(sources[k].mesh_id != s.mesh_id, HK_E_INVALID, "sources %u and %u both name mesh %u", k, i, s.mesh_id);
    HK_REQUIRE(s.positions && s.normals, HK_E_INVALID, "source %u: positions and normals are required", i);
    HK_REQUIRE((s.indices != nullptr) == (decl[i].n_indices != 0u), HK_E_INVALID, "source %u: mesh %u was declared with %u indices, the index array must be %s", i, s.mesh_id,
               decl[i].n_indices, decl[i].n_indices ? "given" : "NULL");
    const uint32_t strides[3] = {s.positions_stride, s.normals_stride, s.uvs_stride}, packed[3] = {12u, 12u, 8u};
    for (int k = 0; k < 3; ++k)
      HK_REQUIRE(strides[k] == 0u || (strides[k] >= packed[k] && strides[k] % 4u == 0u), HK_E_INVALID, "source %u: a stride of %u bytes (0, or a multiple of 4 of at least %u)", i,
                 strides[k], packed[k]);
  }
  {
    const uint32_t unresolved = builder_unresolved_mesh_count(b);
    HK_REQUIRE(unresolved == n, HK_E_INVALID, "the builder holds %u declared meshes that wait for their arrays, the call names %u of them", unresolved, n);
  }
  if (!n) {  // nothing from device memory: this IS hk_add_meshes
    for (uint32_t& v : c->last_add_sources) v = 0u;
    for (double& v : c->last_add_source_ms) v = 0.0;
    return add_body(c, b, tree_mode, plan, nullptr);
  }
  HK_HIP(hipSetDevice(c->device));
  for (uint32_t i = 0; i < n; ++i) {
    const HkMeshSource& s = sources[i];
    const size_t last = decl[i].n_vertices - 1u;
    if ((rc = check_source(c, i, "positions", s.positions, 4, last * stride_of(s.positions_stride, 12u) + 12u))) return rc;
    if ((rc = check_source(c, i, "normals", s.normals, 4, last * stride_of(s.normals_stride, 12u) + 12u))) return rc;
    if (s.uvs && (rc = check_source(c, i, "uvs", s.uvs, 4, last * stride_of(s.uvs_stride, 8u) + 8u))) return rc;
    if (s.indices && (rc = check_source(c, i, "indices", s.indices, 4, (size_t)decl[i].n_indices * 4u))) return rc;
  }
  // ---- phase 1: the block - status | HkPrimitive records | HkVertex records, the sources in ascending mesh id so that neighbours in the
  // builder are neighbours here - and the launch
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return sources[x].mesh_id < sources[y].mesh_id; });
  size_t total_tris = 0, total_verts = 0, n_tri_blocks = 0, n_vert_blocks = 0;
  for (uint32_t i = 0; i < n; ++i) {
    total_tris += decl[i].n_triangles;
    total_verts += decl[i].n_vertices;
    n_tri_blocks += (decl[i].n_triangles + 255u) / 256u;
    n_vert_blocks += (decl[i].n_vertices + 255u) / 256u;
  }
  HK_REQUIRE(n_tri_blocks + n_vert_blocks <= 0x7FFFFFFFull, HK_E_INVALID, "more geometry than one launch takes");
  constexpr size_t HEAD = 256;
  const size_t block_bytes = HEAD + total_tris * sizeof(HkPrimitive) + total_verts * sizeof(HkVertex);
  if (block_bytes > c->add_block_cap) {
    void* mem = nullptr;
    HK_REQUIRE(hipMalloc(&mem, block_bytes + block_bytes / 4) == hipSuccess, HK_E_NOMEM, "device allocation of %zu bytes failed", block_bytes + block_bytes / 4);
    if (c->add_block) {  // (an append enqueued earlier may still read the old one - on the main stream: it goes once an event behind that has passed)
      hipEvent_t done = nullptr;
      if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess || hipEventRecord(done, c->stream) != hipSuccess) {
        if (done) (void)hipEventDestroy(done);
        (void)hipFree(mem);
        HK_REQUIRE(false, HK_E_HIP, "no event for the retired device block: %s", hipGetErrorString(hipGetLastError()));
      }
      retire(c, c->add_block, done);
    }
    c->add_block = mem;
    c->add_block_cap = block_bytes + block_bytes / 4;
  }
  hipStream_t producer = (hipStream_t)producer_stream;
  if (producer)
    for (hipEvent_t* e : {&c->add_src_ready, &c->add_src_read})
      if (!*e) HK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  if (c->time_add_sources)  // (HK_DEBUG_OPT_ADD_SOURCE_TIMES: a product call creates and records no timed event)
    for (hipEvent_t& e : c->add_ev)
      if (!e) HK_HIP(hipEventCreate(&e));
  uint8_t* block = (uint8_t*)c->add_block;
  // ONE pinned buffer for the call, taken before anything is enqueued and kept to its end: item table | workgroup table | the read-back
  auto al256 = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  const size_t table_bytes = al256(n * sizeof(MeshSourceItem)), seg_bytes = al256((n_tri_blocks + n_vert_blocks) * sizeof(SegmentBlock));
  uint8_t* st = nullptr;
  int k = 0;
  if ((rc = stage(c, table_bytes + seg_bytes + block_bytes, &st, &k))) return rc;
  MeshSourceItem* table = (MeshSourceItem*)st;
  SegmentBlock* blocks = (SegmentBlock*)(st + table_bytes);
  uint8_t* back = st + table_bytes + seg_bytes;
  DeviceRecords records;
  struct Offsets { size_t prims, verts; };
  std::vector<Offsets> where(n);  // (of source i in the block - and in its read-back: kept on the host, the tables are the device's to read)
  {
    size_t p_at = HEAD, v_at = HEAD + total_tris * sizeof(HkPrimitive), tb = 0, vb = n_tri_blocks;
    for (uint32_t i : order) {  // (table[i] stays source i: the status names the caller's index)
      const HkMeshSource& s = sources[i];
      MeshSourceItem d{};
      d.positions = (const uint8_t*)s.positions;
      d.normals = (const uint8_t*)s.normals;
      d.uvs = (const uint8_t*)s.uvs;
      d.indices = (const uint32_t*)s.indices;
      d.prims = (uint4*)(block + p_at);
      d.verts = (uint4*)(block + v_at);
      d.n_vertices = decl[i].n_vertices;
      d.n_tris = decl[i].n_triangles;
      d.stride_p = stride_of(s.positions_stride, 12u);
      d.stride_n = stride_of(s.normals_stride, 12u);
      d.stride_uv = stride_of(s.uvs_stride, 8u);
      d.strip = decl[i].topology == HK_TOPOLOGY_TRIANGLE_STRIP ? 1u : 0u;
      table[i] = d;
      where[i] = Offsets{p_at, v_at};
      records.at.push_back(DeviceRecords::At{s.mesh_id, d.prims, d.verts});
      for (uint32_t first = 0; first < d.n_tris; first += 256u) blocks[tb++] = SegmentBlock{i, first};
      for (uint32_t first = 0; first < d.n_vertices; first += 256u) blocks[vb++] = SegmentBlock{i, first};
      p_at += (size_t)d.n_tris * sizeof(HkPrimitive);
      v_at += (size_t)d.n_vertices * sizeof(HkVertex);
    }
  }
  // ---- nothing above has enqueued anything.  From here on a HIP failure waits for the stream before it returns: what was enqueued has
  // then read the sources and the tables, so the producer needs no event and the staging buffer is free again
  const bool timed = c->time_add_sources;
  uint32_t* d_status = (uint32_t*)block;
  uint32_t launches = 0;
  const double t0 = now_ms();
  auto enqueue = [&]() -> hipError_t {
    hipError_t e;
    if (producer) {  // what the producer has enqueued on the sources so far comes first; it may write them again once the launch has read them
      if ((e = hipEventRecord(c->add_src_ready, producer)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(c->stream, c->add_src_ready, 0)) != hipSuccess) return e;
    }
    if ((e = hipMemsetAsync(d_status, 0xFF, 16, c->stream)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(c->add_ev[0], c->stream)) != hipSuccess) return e;
    launches = launch_assemble_meshes(c->stream, table, blocks, (uint32_t)n_tri_blocks, (uint32_t)(n_tri_blocks + n_vert_blocks), d_status, producer ? c->add_src_read : nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(c->add_ev[1], c->stream)) != hipSuccess) return e;
    if (producer && (e = hipStreamWaitEvent(producer, c->add_src_read, 0)) != hipSuccess) return e;
    // the one wait (hk_add_meshes waits for its own build anyway): status and records come back in one copy
    if ((e = hipMemcpyAsync(back, block, block_bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
  };
  {
    const hipError_t e = enqueue();
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(c->stream);
      (void)hipGetLastError();
      HK_REQUIRE(false, HK_E_HIP, "assembling the meshes from device memory failed: %s", hipGetErrorString(e));
    }
  }
  const double t1 = now_ms();
  const uint32_t status = *(const uint32_t*)back;
  HK_REQUIRE(status == HK_U32_MAX, HK_E_INVALID, "source %u: a vertex index out of range (mesh %u has %u vertices)", status, status < n ? sources[status].mesh_id : 0u,
             status < n ? decl[status].n_vertices : 0u);
  // ---- phase 2: the builder takes the records (it was finished and stays so: the ranges are patched in place)
  for (uint32_t i = 0; i < n; ++i) {
    // (no stand-in over the real boxes: phase 3 builds every pending tree at once, the host's completions from the primitives)
    if ((rc = builder_store_mesh_geometry(b, sources[i].mesh_id, (const HkVertex*)(back + where[i].verts), decl[i].n_vertices, (const HkPrimitive*)(back + where[i].prims),
                                          decl[i].n_triangles, false)))
      return rc;
  }
  // (the stream has been waited for: the staging buffer, never marked pending, is the pool's again - phase 3 may take it)
  if ((rc = hk_scene_builder_vertices(b, &plan.bv, &plan.nv))) return rc;
  if ((rc = hk_scene_builder_primitives(b, &plan.bp, &plan.np))) return rc;
  if ((rc = hk_scene_builder_asset_nodes(b, &plan.bn, &plan.nn))) return rc;
  const double t2 = now_ms();
  c->last_add_sources[0] = n;
  c->last_add_sources[1] = (uint32_t)std::min<size_t>(total_tris, 0xFFFFFFFFull);
  c->last_add_sources[2] = launches;
  c->last_add_sources[3] = 0u;
  float span = 0.0f;
  if (timed && hipEventElapsedTime(&span, c->add_ev[0], c->add_ev[1]) != hipSuccess) (void)hipGetLastError();
  c->last_add_source_ms[0] = span;
  c->last_add_source_ms[1] = t1 - t0;
  c->last_add_source_ms[2] = t2 - t1;
  // ---- phase 3
  return add_body(c, b, tree_mode, plan, &records);
}

// Test hook (hikari_hip_debug.h): what the last hk_add_meshes / hk_add_meshes_device took from device memory and what it staged
int hk_debug_last_add_sources(hk_ctx* c, uint32_t out[4]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = c->last_add_sources[k];
  return HK_OK;
}
// Measurement hook (hikari_hip_debug.h): the phase-1 launch between its events, the wait with the read-back, the builder's store; ms
int hk_debug_last_add_source_times(hk_ctx* c, double out[3]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 3; ++k) out[k] = c->last_add_source_ms[k];
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
