// scene_load.hip - mesh trees built on the device at scene load (hikari_hip.h hk_load_scene; kernels in kernels_tree.hip).
// The reference prepares an arriving mesh on the CPU (mesh.rs:76-166: `bvh` 0.7.1 BVH::build on one thread).  A builder may instead
// hold DEFERRED meshes (hk_scene_builder_add_mesh_deferred: a valid stand-in tree of the final size); hk_load_scene uploads such a
// builder, builds every deferred tree on the device - all meshes below 32 768 triangles together, as a forest, at a number of launches
// that does not depend on how many there are - straight into the mesh-level region in every ordering the scene keeps, and writes the
// trees back into the builder and the context's mirror in reference form.  What it leaves is what hk_upload_scene leaves.
#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

namespace {
constexpr uint32_t FOREST_BATCH_TRIANGLES = 1u << 19;  // triangles built at once: about 460 B of scratch each (240 MB), whatever the scene


// reference form (hikari_hip.h HkNode: leaf boxes empty, every leaf behind a navigator of its own) of ordering 0 of a mesh tree as
// k_forest_emit / k_lbvh_emit write it: the navigator of a leaf carries the leaf's entry, and the leaf slot the same record
bool unfold_mesh_nodes(const HkNode* dev, uint32_t count, uint32_t n_tris, HkNode* out) {
  const float inf = INFINITY;
  auto leaf = [&](uint32_t i) { return dev[i].entry_index >= HK_BVH_LEAF_FLAG; };
  auto empty_leaf = [&](uint32_t entry, uint32_t exit_) {
    HkNode n;
    for (int k = 0; k < 3; ++k) { n.min[k] = inf; n.max[k] = -inf; }
    n.entry_index = entry;
    n.exit_index = exit_;
    return n;
  };
  if (count != 3u * n_tris - 2u) return false;
  if (count == 1u) {
    if (!leaf(0) || dev[0].entry_index - HK_BVH_LEAF_FLAG != 0u || dev[0].exit_index != 1u) return false;
    out[0] = empty_leaf(dev[0].entry_index, 1u);
    return true;
  }
  uint32_t leaves = 0;
  for (uint32_t i = 0; i < count;) {
    if (!leaf(i)) {
      if (dev[i].entry_index != i + 1u || dev[i].exit_index <= i + 1u || dev[i].exit_index > count) return false;
      out[i] = dev[i];
      i += 1u;
      continue;
    }
    // a folded navigator and the leaf slot behind it
    if (i + 1u >= count || dev[i + 1u].entry_index != dev[i].entry_index || dev[i].exit_index != i + 2u || dev[i + 1u].exit_index != i + 2u ||
        dev[i].entry_index - HK_BVH_LEAF_FLAG >= n_tris)
      return false;
    out[i] = dev[i];
    out[i].entry_index = i + 1u;
    out[i + 1u] = empty_leaf(dev[i].entry_index, i + 2u);
    leaves += 1u;
    i += 2u;
  }
  return leaves == n_tris;
}

int grow_scratch(hk_ctx* c, size_t need) {
  if (need <= c->lbvh_scratch_cap) return HK_OK;
  void* mem = nullptr;
  HK_HIP(hipMalloc(&mem, need));
  if (c->lbvh_scratch) {  // (what is enqueued may still use the old one - on the main stream only: it goes once an event behind that has passed)
    hipEvent_t done = nullptr;
    if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess || hipEventRecord(done, c->stream) != hipSuccess) {
      if (done) (void)hipEventDestroy(done);
      (void)hipFree(mem);
      HK_REQUIRE(false, HK_E_HIP, "no event for the retired build scratch: %s", hipGetErrorString(hipGetLastError()));
    }
    retire(c, c->lbvh_scratch, done);
  }
  c->lbvh_scratch = mem;
  c->lbvh_scratch_cap = need;
  return HK_OK;
}
}  // namespace

// the trees of `meshes` built into their ranges of the mesh-level region, then read back into the builder and the mirror
int hk::build_on_device(hk_ctx* c, hk_scene_builder* b, const std::vector<LoadMesh>& meshes, uint32_t mode, uint32_t* launches, bool reference_if_unused) {
  const int build = mode == HK_TREE_SAH ? 1 : 0;
  const uint32_t orderings = c->threaded ? 8u : 1u;
  const size_t n_nodes = c->asset_nodes.size(), n_prims = c->primitives.size(), stride = c->mesh.node_cap;
  std::vector<const LoadMesh*> small, large;
  for (const LoadMesh& m : meshes) {
    HK_REQUIRE((size_t)m.index.node_offset + m.index.node_count <= n_nodes && (size_t)m.index.primitive + m.n_tris <= n_prims && m.index.node_count == 3u * m.n_tris - 2u,
               HK_E_INVALID, "the record of mesh %u lies outside the uploaded mesh arrays", m.id);
    (m.n_tris <= HK_FOREST_MESH_MAX_TRIANGLES ? small : large).push_back(&m);
  }
  // batches of the forest: whole meshes, at most FOREST_BATCH_TRIANGLES triangles each
  std::vector<std::vector<ForestMesh>> batches;
  std::vector<uint32_t> batch_tris;
  for (const LoadMesh* m : small) {
    if (batches.empty() || batch_tris.back() + m->n_tris > FOREST_BATCH_TRIANGLES) {
      batches.emplace_back();
      batch_tris.push_back(0u);
    }
    batches.back().push_back(ForestMesh{batch_tris.back(), m->n_tris, m->index.primitive, m->index.node_offset});
    batch_tris.back() += m->n_tris;
  }
  size_t need = 0;
  for (size_t k = 0; k < batches.size(); ++k) need = std::max(need, forest_scratch_bytes(batch_tris[k], (uint32_t)batches[k].size(), build));
  auto boxes_at = [](uint32_t n) { return (lbvh_scratch_bytes(n) + 255) & ~(size_t)255; };
  for (const LoadMesh* m : large) need = std::max(need, boxes_at(m->n_tris) + 2 * (size_t)m->n_tris * 16);
  int rc;
  double t0 = now_ms();
  if ((rc = grow_scratch(c, need))) return rc;
  if ((rc = join_all(c))) return rc;  // (the mesh-level region has one copy)
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  uint8_t* sbase = c->scene_mem + slots;
  float4* nodes = (float4*)(sbase + c->mesh.nodes);
  const float4 *v0 = (const float4*)(sbase + c->mesh.v0), *v1 = (const float4*)(sbase + c->mesh.v1), *v2 = (const float4*)(sbase + c->mesh.v2);
  for (size_t k = 0; k < batches.size(); ++k)
    HK_REQUIRE(launch_forest_build(c->stream, build, batches[k].data(), (uint32_t)batches[k].size(), batch_tris[k], v0, v1, v2, c->lbvh_scratch, nodes, orderings, 2 * stride,
                                   launches) == 0,
               HK_E_HIP, "device build of the mesh trees failed: %s", hipGetErrorString(hipGetLastError()));
  for (const LoadMesh* m : large) {  // (from SAH_WIDE_MIN triangles a mesh has the whole chip to itself: the build of hk_rebuild_mesh_tree)
    float4* tri_lo = (float4*)((uint8_t*)c->lbvh_scratch + boxes_at(m->n_tris));
    float4* tri_hi = tri_lo + m->n_tris;
    const uint32_t p0 = m->index.primitive;
    launch_mesh_triangle_boxes(c->stream, v0 + p0, v1 + p0, v2 + p0, m->n_tris, tri_lo, tri_hi);
    *launches += 1u;
    float4* lo = nodes + 2 * (size_t)m->index.node_offset;
    TreeBuild tree;  // over the boxes just made, into the mesh's node range of every ordering; nothing keeps the topology
    tree.mode = build;
    tree.n = m->n_tris;
    tree.box_lo = tri_lo; tree.box_hi = tri_hi;
    tree.lo = lo; tree.hi = lo + 1; tree.stride = 2u;
    tree.orderings = orderings; tree.ord_stride = 2 * stride;
    tree.mesh_tree = true;
    tree.one_workgroup_top = c->mesh_rebuild_one_workgroup;
    tree.scratch = c->lbvh_scratch;
    tree.launches = launches;
    HK_REQUIRE(launch_tree_build(c->stream, tree) == 0, HK_E_HIP, "device build of the tree of mesh %u failed: %s", m->id, hipGetErrorString(hipGetLastError()));
  }
  HK_HIP(hipGetLastError());
  HK_HIP(hipStreamSynchronize(c->stream));
  poll_retired(c, false);  // (behind join_all and this wait nothing of the context is in flight: a hipFree waits for nothing)
  c->last_load_ms[3] = now_ms() - t0;
  t0 = now_ms();
  // ---- back to the host: ordering 0 of the span that holds the built ranges, unfolded into the builder and the mirror
  uint32_t span0 = HK_U32_MAX, span1 = 0;
  for (const LoadMesh& m : meshes) {
    span0 = std::min(span0, m.index.node_offset);
    span1 = std::max(span1, m.index.node_offset + m.index.node_count);
  }
  static_assert(sizeof(HkNode) == 32, "HkNode is two float4");
  std::vector<HkNode> dev((size_t)span1 - span0), ref;
  HK_HIP(hipMemcpy(dev.data(), nodes + 2 * (size_t)span0, dev.size() * 32, hipMemcpyDeviceToHost));
  std::vector<uint8_t> used;  // (hk_add_meshes does not ask: its cost must not follow the scene)
  if (reference_if_unused) {
    used.assign(n_nodes + 1, 0);
    for (const HkInstance& in : c->instances)
      if (in.mesh.node_count) used[in.mesh.node_offset] = 1;
  }
  for (const LoadMesh& m : meshes) {
    ref.resize(m.index.node_count);
    HK_REQUIRE(unfold_mesh_nodes(dev.data() + (m.index.node_offset - span0), m.index.node_count, m.n_tris, ref.data()), HK_E_HIP,
               "the device build of mesh %u did not leave a tree in the flatten_custom layout", m.id);
    if ((rc = builder_store_mesh_nodes(b, m.id, ref.data(), m.index.node_count))) return rc;
    std::copy(ref.begin(), ref.end(), c->asset_nodes.begin() + m.index.node_offset);
    if (reference_if_unused && !used[m.index.node_offset])  // no instance carries the mesh yet: the layout keeps such a range in reference form, in every ordering
      for (uint32_t o = 0; o < orderings; ++o)
        HK_HIP(hipMemcpy(nodes + 2 * ((size_t)o * stride + m.index.node_offset), ref.data(), (size_t)m.index.node_count * 32, hipMemcpyHostToDevice));
  }
  c->last_load_ms[4] = now_ms() - t0;
  return HK_OK;
}

extern "C" {

int hk_load_scene(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(tree_mode == HK_TREE_SAH || tree_mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", tree_mode);
  HK_REQUIRE(!builder_has_standin_trees(b), HK_E_NOT_READY,
             "the builder holds stand-in instance trees (hk_scene_builder_finish_instances): finish it with hk_scene_builder_finish before hk_load_scene");
  HK_NO_UNRESOLVED_MESHES(b);  // (declared meshes hold zeros: hk_add_meshes_device or hk_scene_builder_resolve_mesh fills them)
  const HkNode* an = nullptr;
  uint32_t nan_ = 0;
  int rc;
  if ((rc = hk_scene_builder_asset_nodes(b, &an, &nan_))) return rc;  // (HK_E_NOT_READY: not finished)
  std::vector<LoadMesh> device, host;
  for (uint32_t id = 0, n = builder_mesh_count(b); id < n; ++id) {
    LoadMesh m{id, HkMeshIndex{}, 0u};
    if (!builder_pending_mesh(b, id, &m.index)) continue;
    HK_REQUIRE(m.index.node_count >= 1u && (m.index.node_count + 2u) % 3u == 0u, HK_E_INVALID, "mesh %u: a stand-in tree of %u nodes", id, m.index.node_count);
    m.n_tris = (m.index.node_count + 2u) / 3u;
    (m.n_tris > c->load_device_limit ? host : device).push_back(m);
  }
  for (uint32_t& v : c->last_load) v = 0u;
  for (double& v : c->last_load_ms) v = 0.0;
  double t0 = now_ms();
  // meshes beyond what the device build takes are completed by the host's builder: nothing has been uploaded yet
  for (const LoadMesh& m : host)
    if ((rc = builder_complete_mesh_on_host(b, m.id))) return rc;
  c->last_load[3] = (uint32_t)host.size();
  c->last_load_ms[0] = now_ms() - t0;
  if (device.empty()) return hk_upload_scene(c, b);
  c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_HIP(hipSetDevice(c->device));
  t0 = now_ms();
  if ((rc = upload_scene_unchecked(c, b))) return rc;
  c->last_load_ms[1] = now_ms() - t0;
  t0 = now_ms();
  for (const LoadMesh& m : device) c->load_pending_ranges.emplace_back(m.index.node_offset, m.index.node_count);
  rc = finalize_scene(c);  // (the ranges about to be built are neither threaded nor folded on the host)
  c->load_pending_ranges.clear();
  c->last_load_ms[2] = now_ms() - t0;
  uint32_t launches = 0;
  if (!rc) rc = build_on_device(c, b, device, tree_mode, &launches, true);
  if (rc) {  // never a scene with stand-in trees in it: the context is left without one
    c->have_meshes = false;
    c->mesh_dirty = true;
    return rc;
  }
  c->last_load[0] = (uint32_t)device.size();
  for (const LoadMesh& m : device) c->last_load[1] += m.n_tris;
  c->last_load[2] = launches;
  c->device_tree_builds += device.size();
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): what the last hk_load_scene did
int hk_debug_last_load(hk_ctx* c, uint32_t out[4]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = c->last_load[k];
  return HK_OK;
}

// Measurement hook (hikari_hip_debug.h): where the time of the last hk_load_scene went
int hk_debug_last_load_times(hk_ctx* c, double out[5]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 5; ++k) out[k] = c->last_load_ms[k];
  return HK_OK;
}

}  // extern "C"
