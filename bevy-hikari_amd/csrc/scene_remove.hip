// scene_remove.hip - meshes removed from a loaded scene, the mesh-level region compacted on the device (hikari_hip.h hk_remove_meshes;
// kernels in kernels_scene.hip; DESIGN 3 "Meshes that leave").  The twin of scene_append.hip: the scene moves, behind every stream, to a
// NEW allocation sized for the survivors (scene_move.hip) - the destination of every run lies in front of its source, so a move in place would need an
// order across workgroups, frames in flight go on reading the old allocation, and a failure before the switch leaves the scene the
// context had.  One launch moves the surviving runs of every plane however many meshes go; one small launch beside it copies the
// instance-level slot and rebases the three words of every instance record that name mesh offsets; a copy launch in front of both takes
// the plan from pinned to device memory.  Links and leaf ids are local to a mesh: nothing inside a tree, a wide record or a rank changes.
#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

namespace {
struct Entry { HkMeshExtent e; uint32_t index; };   // index: the entry's position in the caller's array (for the error text)

// the surviving intervals of [0, size) once the sorted, disjoint ranges (begin, count) are gone, with their prefix sum
std::vector<CompactRun> surviving_runs(const std::vector<std::pair<uint32_t, uint32_t>>& gone, uint32_t size) {
  std::vector<CompactRun> runs;
  uint32_t at = 0, dst = 0;
  auto add = [&](uint32_t end) {
    if (end > at) {
      runs.push_back(CompactRun{at, dst, end - at, 0u});
      dst += end - at;
    }
  };
  for (const auto& g : gone) {
    add(g.first);
    at = g.first + g.second;
  }
  add(size);
  return runs;
}
uint32_t survivors(const std::vector<CompactRun>& runs) { return runs.empty() ? 0u : runs.back().dst + runs.back().count; }
// the ranges erased from a mirror, back to front
template <typename T>
void erase_ranges(std::vector<T>& v, const std::vector<std::pair<uint32_t, uint32_t>>& gone) {
  size_t to = 0, at = 0;
  for (const auto& g : gone) {
    if (to != at) std::move(v.begin() + at, v.begin() + g.first, v.begin() + to);
    to += g.first - at;
    at = (size_t)g.first + g.second;
  }
  if (to != at) std::move(v.begin() + at, v.end(), v.begin() + to);
  v.resize(to + (v.size() - at));
}
HkMeshIndex rebased(const std::vector<CompactRun> runs[3], HkMeshIndex m) {
  m.node_offset = compact_rebase(runs[0].data(), (uint32_t)runs[0].size(), m.node_offset);
  m.primitive = compact_rebase(runs[1].data(), (uint32_t)runs[1].size(), m.primitive);
  m.vertex = compact_rebase(runs[2].data(), (uint32_t)runs[2].size(), m.vertex);
  return m;
}
// the host state once the meshes are gone: mirrors compacted, instance records (and the laid-out copy of them the next diff reads),
// wide bookkeeping and deformable meshes re-keyed
void compact_host_state(hk_ctx* c, const std::vector<std::pair<uint32_t, uint32_t>> gone[3], const std::vector<CompactRun> runs[3], std::vector<void*>& freed) {
  const bool have_prim_offsets = c->node_prim_offset.size() == c->asset_nodes.size();  // (the layout's note of the primitives a node's leaves index)
  erase_ranges(c->asset_nodes, gone[0]);
  if (have_prim_offsets) {
    erase_ranges(c->node_prim_offset, gone[0]);
    for (int64_t& p : c->node_prim_offset)
      if (p >= 0) p = (int64_t)compact_rebase(runs[1].data(), (uint32_t)runs[1].size(), (uint32_t)p);
  }
  erase_ranges(c->primitives, gone[1]);
  erase_ranges(c->vertices, gone[2]);
  for (HkInstance& in : c->instances) in.mesh = rebased(runs, in.mesh);
  const size_t first = c->dyn_off.instances, n_inst = c->instances.size();
  if (first + n_inst * sizeof(DInstance) <= c->dyn_blob.bytes.size())
    for (size_t i = 0; i < n_inst; ++i) {
      DInstance d;
      memcpy(&d, c->dyn_blob.bytes.data() + first + i * sizeof(DInstance), sizeof(DInstance));
      d.node_offset = compact_rebase(runs[0].data(), (uint32_t)runs[0].size(), d.node_offset);
      d.primitive = compact_rebase(runs[1].data(), (uint32_t)runs[1].size(), d.primitive);
      d.vertex = compact_rebase(runs[2].data(), (uint32_t)runs[2].size(), d.vertex);
      memcpy(c->dyn_blob.bytes.data() + first + i * sizeof(DInstance), &d, sizeof(DInstance));
    }
  std::vector<std::pair<uint32_t, uint32_t>> wide;
  for (const auto& m : c->wide_meshes) {
    bool survives = false;
    for (const CompactRun& r : runs[0]) survives = survives || (m.first >= r.src && m.first - r.src < r.count);
    if (survives) wide.emplace_back(compact_rebase(runs[0].data(), (uint32_t)runs[0].size(), m.first), m.second);
  }
  c->wide_meshes.swap(wide);  // (the rebase is monotonic: still sorted)
  rebase_deform_meshes(c, runs, freed);
}
}  // namespace

extern "C" {

int hk_remove_meshes(hk_ctx* c, const HkMeshExtent* removed, uint32_t n) {
  HK_REQUIRE(c && (removed || !n), HK_E_INVALID, "NULL argument");
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene or hk_load_scene must come first");
  // ---- validation: nothing is written or enqueued before all of it has passed
  const size_t n_nodes = c->asset_nodes.size(), n_prims = c->primitives.size(), n_verts = c->vertices.size();
  std::vector<Entry> ext;
  for (uint32_t i = 0; i < n; ++i) {
    const HkMeshExtent& e = removed[i];
    if (!e.node_count) continue;  // (a mesh no finish of the builder had seen: the context never held it)
    HK_REQUIRE(e.n_primitives != 0 && e.node_count == 3u * e.n_primitives - 2u && (uint64_t)e.node_count == 3ull * e.n_primitives - 2ull, HK_E_INVALID,
               "entry %u: %u nodes for %u triangles (a mesh tree has 3 n - 2)", i, e.node_count, e.n_primitives);
    HK_REQUIRE((size_t)e.node_offset + e.node_count <= n_nodes && (size_t)e.primitive + e.n_primitives <= n_prims && (size_t)e.vertex + e.n_vertices <= n_verts, HK_E_INVALID,
               "entry %u: the extent (%u + %u vertices, %u + %u primitives, %u + %u nodes) leaves the uploaded mesh arrays (%zu, %zu, %zu)", i, e.vertex, e.n_vertices,
               e.primitive, e.n_primitives, e.node_offset, e.node_count, n_verts, n_prims, n_nodes);
    ext.push_back(Entry{e, i});
  }
  if (ext.empty()) {  // nothing to do: nothing is enqueued
    for (uint64_t& v : c->last_remove) v = 0;
    c->rm_timed = false;
    return HK_OK;
  }
  std::stable_sort(ext.begin(), ext.end(), [](const Entry& a, const Entry& b) { return a.e.node_offset < b.e.node_offset; });
  for (size_t k = 0; k + 1 < ext.size(); ++k) {
    const HkMeshExtent &a = ext[k].e, &b = ext[k + 1].e;
    HK_REQUIRE((uint64_t)a.node_offset + a.node_count <= b.node_offset && (uint64_t)a.primitive + a.n_primitives <= b.primitive && (uint64_t)a.vertex + a.n_vertices <= b.vertex,
               HK_E_INVALID, "entry %u: the extent overlaps entry %u, or the two are ordered differently in nodes, primitives and vertices", ext[k + 1].index, ext[k].index);
  }
  std::vector<std::pair<uint32_t, uint32_t>> gone[3];
  for (const Entry& x : ext) {
    gone[0].emplace_back(x.e.node_offset, x.e.node_count);
    gone[1].emplace_back(x.e.primitive, x.e.n_primitives);
    gone[2].emplace_back(x.e.vertex, x.e.n_vertices);
  }
  // which entry holds, or cuts, the range [begin, begin + count) of list l: -1 none, else its position in ext; *whole: it lies inside
  auto touches = [&](int l, uint64_t begin, uint64_t count, bool* whole) -> int {
    const auto& g = gone[l];
    size_t lo = 0, hi = g.size();   // the first extent that ends behind `begin`
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if ((uint64_t)g[mid].first + g[mid].second <= begin) lo = mid + 1; else hi = mid;
    }
    if (lo == g.size() || (uint64_t)g[lo].first >= begin + std::max<uint64_t>(count, 1)) return -1;
    *whole = g[lo].first <= begin && begin + count <= (uint64_t)g[lo].first + g[lo].second;
    return (int)lo;
  };
  for (size_t i = 0; i < c->instances.size(); ++i) {  // (the mirror of the instance SET is authoritative even where poses and boxes are stale)
    const HkMeshIndex& m = c->instances[i].mesh;
    bool whole = false;
    int at = touches(0, m.node_offset, m.node_count, &whole);
    if (at < 0) at = touches(1, m.primitive, (m.node_count + 2u) / 3u, &whole);
    if (at < 0) at = touches(2, m.vertex, 1, &whole);
    HK_REQUIRE(at < 0, HK_E_INVALID, "entry %u: uploaded instance %zu still uses the mesh (%u, %u, %u, %u): remove its instances first (hk_update_scene_instances)",
               ext[(size_t)at].index, i, m.vertex, m.primitive, m.node_offset, m.node_count);
  }
  {
    std::vector<HkMeshIndex> known;
    deform_mesh_records(c, known);
    for (const HkMeshIndex& m : known) {
      bool w0 = true, w1 = true, w2 = true;
      const int a0 = touches(0, m.node_offset, m.node_count, &w0), a1 = touches(1, m.primitive, (m.node_count + 2u) / 3u, &w1), a2 = touches(2, m.vertex, 1, &w2);
      const int at = a0 >= 0 ? a0 : a1 >= 0 ? a1 : a2;
      HK_REQUIRE(at < 0 || (a0 == a1 && a1 == a2 && w0 && w1 && w2), HK_E_INVALID, "entry %u: the extent cuts the deformable mesh (%u, %u, %u, %u)", ext[(size_t)std::max(at, 0)].index,
                 m.vertex, m.primitive, m.node_offset, m.node_count);
    }
    for (const auto& m : c->wide_meshes) {
      bool whole = true;
      const int at = touches(0, m.first, m.second, &whole);
      HK_REQUIRE(at < 0 || whole, HK_E_INVALID, "entry %u: the extent cuts the mesh tree [%u, +%u)", ext[(size_t)std::max(at, 0)].index, m.first, m.second);
    }
  }
  std::vector<CompactRun> runs[3] = {surviving_runs(gone[0], (uint32_t)n_nodes), surviving_runs(gone[1], (uint32_t)n_prims), surviving_runs(gone[2], (uint32_t)n_verts)};
  const size_t now_nodes = survivors(runs[0]), now_prims = survivors(runs[1]), now_verts = survivors(runs[2]);
  HK_REQUIRE(now_nodes && now_prims && now_verts, HK_E_INVALID, "entry %u: no mesh would be left", ext[0].index);
  uint64_t tris_removed = 0;
  for (const Entry& x : ext) tris_removed += x.e.n_primitives;
  // ---- every check of the arguments has passed (a refusal above leaves the report of the last removal as it was)
  // (... and so does the refusal of the full layout below: the report is cleared behind the last refusal)
  auto clear_report = [&] {
    for (uint64_t& v : c->last_remove) v = 0;
    c->rm_timed = false;
  };

  HK_HIP(hipSetDevice(c->device));
  int rc;
  std::vector<void*> freed;
  const bool laid_out = !c->mesh_dirty && c->scene_mem;
  if (laid_out && (rc = finalize_scene(c))) return rc;  // (a pending instance-level layout first; refused as ever with stale mirrors - nothing changed)
  if (!laid_out || !c->two_slots || wants_threaded(c, now_nodes, now_prims, now_verts) != c->threaded) {
    // ---- the full layout: scenes walked from the LDS copy, removals that change the ordering count (and a scene not laid out yet)
    HK_REQUIRE(!c->mirrors_stale && !c->meshes_deformed, HK_E_NOT_READY,
               "the scene was last changed on the device and this removal lays it out again on the host: upload the host's mirror first (hk_upload_scene)");
    clear_report();
    if ((rc = sync_all(c))) return rc;  // (the deformable meshes that go are freed at once; the layout below waits anyway)
    compact_host_state(c, gone, runs, freed);
    for (void* q : freed) (void)hipFree(q);
    c->scene_epoch += 1;
    c->mesh_dirty = true;
    c->dynamic_dirty = true;
    if ((rc = finalize_scene(c))) return rc;
    c->last_remove[0] = ext.size(); c->last_remove[1] = tris_removed; c->last_remove[3] = runs[0].size(); c->last_remove[4] = 1;
    return HK_OK;
  }

  // ---- the device compaction
  clear_report();
  uint64_t enqueued = 0;  // kernel launches and fills, counted where they are enqueued (hk_debug_last_remove)
  const bool propagate = c->deform_pending;
  if ((rc = flush_deform(c))) return rc;  // (a pending propagate of deformed boxes names the old records: it goes first, in stream order)
  if (propagate) enqueued += c->last_deform[4];
  if (!c->compute_units) {
    hipDeviceProp_t prop;
    HK_HIP(hipGetDeviceProperties(&prop, c->device));
    c->compute_units = prop.multiProcessorCount;
  }
  // the wide records and ranks of the survivors are moved, not derived again - where they exist and describe the scene
  const bool move_wide = c->wide_blas && !c->wide_blas_dirty && c->wide_blas_slots >= n_nodes;
  const bool move_rank = move_wide && c->wide_blas_rank && c->wide_rank_primitives >= n_prims;
  // ---- the plan, in one pinned block: planes, then the three run lists
  size_t run_first[3], table_bytes = HK_COMPACT_PLANES * sizeof(CompactPlane);
  for (int l = 0; l < 3; ++l) { run_first[l] = table_bytes; table_bytes += runs[l].size() * sizeof(CompactRun); }
  table_bytes = (table_bytes + 15) & ~(size_t)15;
  uint8_t* st = nullptr;
  int sk = 0;
  if ((rc = stage(c, table_bytes, &st, &sk))) return rc;
  if ((rc = join_all(c))) return rc;  // (the mesh-level region has one copy: the move goes behind every frame enqueued so far)
  for (int k = 0; k < 2; ++k)
    if (!c->rm_ev[k]) HK_HIP(hipEventCreate(&c->rm_ev[k]));
  SceneMove m;  // (the slots keep their size; the plan's device copy lives as long as the move)
  if ((rc = move_begin(c, move_room(MeshSizes{now_nodes, now_prims, now_verts}), c->dyn_capacity, move_wide, move_rank, table_bytes, "no room for the compacted scene", &m))) return rc;
  enqueued += m.rank ? 1 : 0;  // (the fill of the new ranks)
  CompactArgs a{};
  CompactPlane* planes = (CompactPlane*)st;
  uint64_t moved_bytes = 0;
  bool inside = true;  // every source inside the old capacities, every destination inside the new ones
  MovePlane moving[HK_MOVE_PLANES];
  static_assert(HK_MOVE_PLANES <= HK_COMPACT_PLANES, "the compaction's table holds every plane of a move");
  for (uint32_t k = 0, n_moving = move_planes(c, m, moving); k < n_moving; ++k) {
    const MovePlane& p = moving[k];
    const uint64_t plane_total = (uint64_t)survivors(runs[p.list]) << p.shift;
    for (const CompactRun& r : runs[p.list]) inside = inside && (size_t)r.src + r.count <= p.old_cap && (size_t)r.dst + r.count <= p.new_cap;
    inside = inside && ((uintptr_t)p.src & 15u) == 0 && ((uintptr_t)p.dst & 15u) == 0;
    planes[a.n_planes++] = CompactPlane{p.src, p.dst, p.list, p.shift, a.n_pieces};
    a.n_pieces += (plane_total + HK_COMPACT_PIECE - 1) / HK_COMPACT_PIECE;
    moved_bytes += plane_total;
  }
  for (uint32_t k = a.n_planes; k < HK_COMPACT_PLANES; ++k) planes[k] = CompactPlane{nullptr, nullptr, 0u, 0u, ~0ull};
  a.planes = (const CompactPlane*)m.extra;
  for (int l = 0; l < 3; ++l) {
    memcpy(st + run_first[l], runs[l].data(), runs[l].size() * sizeof(CompactRun));
    a.runs[l] = (const CompactRun*)(m.extra + run_first[l]);
    a.n_runs[l] = (uint32_t)runs[l].size();
    a.total[l] = survivors(runs[l]);
  }
  const size_t first16 = c->dyn_off.instances / 16, n_inst = c->instances.size();
  inside = inside && c->dyn_off.instances % 16 == 0 && c->dyn_off.instances + n_inst * sizeof(DInstance) <= c->dyn_capacity && c->dyn_capacity % 16 == 0;
  if (!inside) {
    move_abort(c, &m, m.rank != nullptr);  // (nothing but the ranks' fill was enqueued)
    HK_REQUIRE(false, HK_E_INVALID, "the compaction plan leaves the scene's capacities");  // (a bug of this file, never of the caller)
  }
  // the table to device memory (a copy kernel reading the pinned block), the planes, the instance-level slot in use into both new slots
  launch_copy_region(c->stream, m.extra, st, table_bytes);
  enqueued += 1;
  bool ok = hipEventRecord(c->rm_ev[0], c->stream) == hipSuccess;
  launch_compact_planes(c->stream, a, c->compute_units);
  enqueued += a.n_pieces ? 1 : 0;
  ok = ok && hipEventRecord(c->rm_ev[1], c->stream) == hipSuccess;
  launch_compact_instances(c->stream, (uint4*)m.mem, (uint4*)(m.mem + c->dyn_capacity), (const uint4*)(c->scene_mem + (size_t)c->slot * c->dyn_capacity), c->dyn_capacity / 16,
                           first16, (uint32_t)n_inst, a);
  enqueued += c->dyn_capacity / 16 ? 1 : 0;
  if (!ok || hipGetLastError() != hipSuccess) {
    const hipError_t e = hipGetLastError();
    move_abort(c, &m, true);  // (the move may be enqueued)
    HK_REQUIRE(false, HK_E_HIP, "the compaction of the scene failed: %s", hipGetErrorString(e));
  }
  if ((rc = move_commit(c, &m, 0))) return rc;  // (slot 0: both slots hold the instance level as it stands)
  hk_ctx::DeformStage& ds = c->df_stage[(size_t)sk];
  if (hipEventRecord(ds.done, c->stream) == hipSuccess) ds.pending = true;
  else (void)hipStreamSynchronize(c->stream);  // (no event: the pinned plan has been read once the stream is idle)
  c->rm_timed = true;
  if (c->wide_blas && !move_wide) c->wide_blas_dirty = true;  // (records that did not describe the scene: derived again for the new layout)
  if (c->wide_blas_rank && !move_rank) c->wide_blas_dirty = true;
  c->scene_epoch += 1;  // (scene memory was written: hk_context.hpp, primary-ray pipelining)
  compact_host_state(c, gone, runs, freed);
  for (void* q : freed) {  // what the removed deformable meshes held: frames in flight may still use it
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess && hipEventRecord(e, c->stream) == hipSuccess) retire(c, q, e);
    else if (e) (void)hipEventDestroy(e);  // (no event: the allocation stays until the context goes)
  }
  c->last_remove[0] = ext.size(); c->last_remove[1] = tris_removed; c->last_remove[2] = enqueued; c->last_remove[3] = runs[0].size(); c->last_remove[4] = 0;
  c->last_remove[5] = moved_bytes;
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): what the last hk_remove_meshes did
int hk_debug_last_remove(hk_ctx* c, uint64_t out[6]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 6; ++k) out[k] = c->last_remove[k];
  return HK_OK;
}
// Measurement hook (hikari_hip_debug.h): the compaction launch of the last hk_remove_meshes between two events
int hk_debug_last_remove_ms(hk_ctx* c, float* ms) {
  HK_REQUIRE(c && ms, HK_E_INVALID, "NULL argument");
  *ms = 0.0f;
  if (!c->rm_timed) return HK_OK;
  HK_HIP(hipEventSynchronize(c->rm_ev[1]));
  HK_HIP(hipEventElapsedTime(ms, c->rm_ev[0], c->rm_ev[1]));
  return HK_OK;
}

}  // extern "C"
