// scene_refit.hip - instance motion and instance-set changes on the device (kernels in kernels_scene.hip, tree builds in kernels_tree.hip): the
// reference re-runs prepare_instances on the host for ANY instance change (instance.rs:352-437); here moved instances are refit,
// both trees rebuilt (the reference's SAH tree or an LBVH) and instance-set edits laid out without the host's two tree builds.
#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

extern "C" {

// Instances added, removed or re-materialed (the reference re-runs prepare_instances for ANY instance change, instance.rs:352-437):
// the per-instance / per-emitter records are laid out on the host - O(instances), no tree build - and go to the spare slot through
// the asynchronous upload; both trees are then built on the device (hk_rebuild_scene_trees: HK_TREE_SAH = the reference's own
// tree, link for link).  What the host no longer does is the two `BVH::build` calls: 1.1 ms of 1.7 ms at 2 000 instances, 30 of
// 32 ms at 20 000.
int hk_update_scene_instances(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(tree_mode == HK_TREE_SAH || tree_mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", tree_mode);
  HK_REQUIRE(!c->meshes_deformed, HK_E_NOT_READY, "a mesh was deformed on the device: upload the host's mirror of it (hk_upload_scene) first");
  HK_NO_PENDING_MESHES(b);  // (before the builder is finished: a refusal changes nothing)
  int rc;
  const bool trace = c->trace_update;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  if ((rc = hk_scene_builder_finish_instances(b))) return rc;
  const double t1 = now();
  const size_t n_materials = c->materials.size();
  if ((rc = take_appended_materials(c, b))) return rc;  // (a spawned object is a mesh, a material and an instance; refused ids write nothing)
  if ((rc = upload_scene_instances_unchecked(c, b))) {  // (refused: the material mirror is what it was)
    c->materials.resize(n_materials);
    return rc;
  }
  const double t2 = now();
  uint32_t ni = 0;
  const HkInstance* inst = nullptr;
  if ((rc = hk_scene_builder_instances(b, &inst, &ni))) return rc;
  c->trees_pending_on_device = ni >= 2;
  rc = finalize_scene(c);
  c->trees_pending_on_device = false;
  const double t3 = now();
  if (!rc && ni >= 2) rc = hk_rebuild_scene_trees(c, tree_mode);  // (a tree of one leaf is what the host just laid out)
  // the region just uploaded carries stand-in trees with orderings 1..7 left zero (the device build was to overwrite
  // them in stream order).  If that build did not get enqueued, a threaded walk over zero nodes would never leave node 0: the
  // next use of the scene lays the region out again, from the host's (valid) stand-in trees, all orderings threaded.
  if (rc) c->dynamic_dirty = true;
  if (trace) fprintf(stderr, "hk_update_scene_instances: finish_instances %.2f ms, mirrors %.2f ms, layout + upload %.2f ms, device build enqueue %.2f ms\n", t1 - t0, t2 - t1, t3 - t2, now() - t3);
  return rc;
}

// ---- instance motion on the device (kernels_scene.hip) --------------------------------------------------
}  // extern "C"
namespace hk {
void free_refit(hk_ctx* c) {
  for (void* q : {(void*)c->rf_inst_lo, (void*)c->rf_inst_hi, (void*)c->rf_prev_models, (void*)c->rf_emissive_of_instance, (void*)c->rf_alias_scratch})
    if (q) (void)hipFree(q);
  c->rf_inst_lo = c->rf_inst_hi = c->rf_prev_models = nullptr;
  c->rf_emissive_of_instance = nullptr;
  c->rf_alias_scratch = nullptr;
  c->rf_instances = c->rf_alias = 0;
  c->rf_ready = false;
  if (c->lbvh_scratch) (void)hipFree(c->lbvh_scratch);
  c->lbvh_scratch = nullptr;
  c->lbvh_scratch_cap = 0;
  for (int k = 0; k < 2; ++k) {
    if (c->mt_updates[k]) (void)hipHostFree(c->mt_updates[k]);
    if (c->mt_done[k]) (void)hipEventDestroy(c->mt_done[k]);
    c->mt_updates[k] = nullptr;
    c->mt_done[k] = nullptr;
    c->mt_updates_cap[k] = 0;
    c->mt_pending[k] = false;
  }
  for (int k = 0; k < 2; ++k) {
    if (c->rf_updates[k]) (void)hipHostFree(c->rf_updates[k]);
    if (c->rf_done[k]) (void)hipEventDestroy(c->rf_done[k]);
    c->rf_updates[k] = nullptr;
    c->rf_done[k] = nullptr;
    c->rf_updates_cap[k] = 0;
    c->rf_pending[k] = false;
  }
}
hkd::RefitScene refit_scene(hk_ctx* c) {
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  hkd::RefitScene r;
  r.instances = (DInstance*)(base + c->dyn_off.instances);
  r.prev_models = c->rf_prev_models;
  r.inst_lo = c->rf_inst_lo;
  r.inst_hi = c->rf_inst_hi;
  r.emissive_of_instance = c->rf_emissive_of_instance;
  r.emissives = (DEmissive*)(base + c->dyn_off.emissives);
  r.alias = (float2*)(base + c->dyn_off.alias);
  r.alias_scratch = c->rf_alias_scratch;
  r.materials = (const float4*)(base + c->dyn_off.materials);
  r.tri_v0 = c->scene.tri_v0;
  r.tri_v1 = c->scene.tri_v1;
  r.tri_v2 = c->scene.tri_v2;
  return r;
}
// side arrays of the refit, (re)filled from the scene as the host last laid it out: world AABB per instance from the TLAS
// leaves, emitter of an instance, previous models
int prepare_refit(hk_ctx* c) {
  if (c->rf_ready) return HK_OK;
  const size_t ni = c->instances.size(), na = c->alias_table.size();
  if (ni > c->rf_instances || na > c->rf_alias) {
    int rc = sync_all(c);
    if (rc) return rc;
    for (void* q : {(void*)c->rf_inst_lo, (void*)c->rf_inst_hi, (void*)c->rf_prev_models, (void*)c->rf_emissive_of_instance, (void*)c->rf_alias_scratch})
      if (q) (void)hipFree(q);
    c->rf_inst_lo = c->rf_inst_hi = c->rf_prev_models = nullptr;
    c->rf_emissive_of_instance = nullptr;
    c->rf_alias_scratch = nullptr;
    c->rf_instances = c->rf_alias = 0;  // (stays 0 if an allocation below fails: the next call starts over)
    const size_t cap_i = ni + ni / 4, cap_a = na + na / 4 + 4;
    HK_HIP(hipMalloc((void**)&c->rf_inst_lo, cap_i * 16));
    HK_HIP(hipMalloc((void**)&c->rf_inst_hi, cap_i * 16));
    HK_HIP(hipMalloc((void**)&c->rf_prev_models, cap_i * 64));
    HK_HIP(hipMalloc((void**)&c->rf_emissive_of_instance, cap_i * 4));
    HK_HIP(hipMalloc((void**)&c->rf_alias_scratch, cap_a * 5 * 4));
    c->rf_instances = cap_i;
    c->rf_alias = cap_a;
  }
  std::vector<uint32_t> eoi(ni, 0xFFFFFFFFu);
  for (size_t e = 0; e < c->emissives.size(); ++e) eoi[c->emissives[e].instance] = (uint32_t)e;
  HK_HIP(hipMemcpyAsync(c->rf_emissive_of_instance, eoi.data(), ni * 4, hipMemcpyHostToDevice, c->stream));
  HK_HIP(hipStreamSynchronize(c->stream));  // (eoi is a local; once per host-side rebuild)
  const hkd::RefitScene r = refit_scene(c);
  const uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  launch_gather_instance_boxes(c->stream, r, (const float4*)(base + c->dyn_off.tlas), (uint32_t)c->instance_nodes.size());
  // previous models of the instances the host marked as moved (the plane exists only then)
  if (c->prev_models.size() == 16 * ni && c->dyn_off.prev_models + ni * 64 <= c->dyn_capacity && c->d_prev_models && c->d_prev_models != c->rf_prev_models) {
    bool any = false;
    for (size_t i = 0; i < ni && !any; ++i) any = memcmp(&c->prev_models[16 * i], c->instances[i].model, 64) != 0;
    if (any) launch_copy_region(c->stream, c->rf_prev_models, base + c->dyn_off.prev_models, ni * 64);
  }
  HK_HIP(hipGetLastError());
  c->rf_last_moved.clear();
  for (size_t i = 0; i < ni; ++i)
    if (c->prev_models.size() == 16 * ni && memcmp(&c->prev_models[16 * i], c->instances[i].model, 64) != 0) c->rf_last_moved.push_back((uint32_t)i);
  c->rf_ready = true;
  return HK_OK;
}
}  // namespace hk
// frames in flight keep reading the slot they were enqueued with: a device-side update works on a copy in the spare slot
// (two-slot scenes), or in place behind everything enqueued so far (scenes small enough for the LDS copy have one slot)
int hk::begin_device_update(hk_ctx* c) {
  const int rc = join_side(c);
  if (rc) return rc;
  if (c->two_slots) {
    uint8_t* from = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
    c->slot ^= 1;
    uint8_t* to = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
    launch_copy_region(c->stream, to, from, c->dyn_capacity);
    const float4* prev = c->d_prev_models;
    point_scene_at_slot(c);
    if (prev == c->rf_prev_models) c->d_prev_models = prev;  // (the refit's own plane is not part of the slot)
  }
  return HK_OK;
}
extern "C" {

int hk_rebuild_scene_trees(hk_ctx* c, uint32_t mode) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c, HK_E_INVALID, "ctx is NULL");
  HK_REQUIRE(mode == HK_TREE_SAH || mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", mode);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = flush_deform(c))) return rc;   // (the trees are built over the instances' current boxes)
  const uint32_t ni = (uint32_t)c->instances.size(), ne = (uint32_t)c->emissives.size();
  HK_REQUIRE(c->instance_nodes.size() == 3 * (size_t)ni - 2 && (ne == 0 || c->emissive_nodes.size() == 3 * (size_t)ne - 2), HK_E_UNSUPPORTED,
             "the uploaded trees are not in the flatten_custom layout of a binary tree (3n - 2 nodes): nothing to rebuild in place");
  if ((rc = prepare_refit(c))) return rc;
  const size_t need = std::max(lbvh_scratch_bytes(ni), lbvh_scratch_bytes(std::max(ne, 1u)));
  if (need > c->lbvh_scratch_cap) {
    if ((rc = sync_all(c))) return rc;
    if (c->lbvh_scratch) (void)hipFree(c->lbvh_scratch);
    c->lbvh_scratch = nullptr;
    c->lbvh_scratch_cap = 0;
    HK_HIP(hipMalloc(&c->lbvh_scratch, need + need / 4));
    c->lbvh_scratch_cap = need + need / 4;
  }
  if ((rc = begin_device_update(c))) return rc;
  const hkd::RefitScene r = refit_scene(c);
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  float4* tlas = (float4*)(base + c->dyn_off.tlas);
  TreeBuild instance_tree;  // over the instances' world boxes, into the interleaved node pairs of every ordering
  instance_tree.mode = mode == HK_TREE_SAH ? 1 : 0;
  instance_tree.n = ni;
  instance_tree.box_lo = c->rf_inst_lo; instance_tree.box_hi = c->rf_inst_hi;
  instance_tree.lo = tlas; instance_tree.hi = tlas + 1; instance_tree.stride = 2u;
  instance_tree.orderings = c->threaded ? 8u : 1u;
  instance_tree.scratch = c->lbvh_scratch;
  HK_REQUIRE(launch_tree_build(c->stream, instance_tree) == 0, HK_E_HIP, "device build of the instance tree failed: %s", hipGetErrorString(hipGetLastError()));
  if (ne) {
    TreeBuild light_tree;  // over the emitters of the scene, into the two planes of the light tree's one ordering
    light_tree.mode = instance_tree.mode;
    light_tree.n = ne;
    light_tree.scene = &r;
    light_tree.lo = (float4*)(base + c->dyn_off.light_lo); light_tree.hi = (float4*)(base + c->dyn_off.light_hi); light_tree.stride = 1u;
    light_tree.scratch = c->lbvh_scratch;
    HK_REQUIRE(launch_tree_build(c->stream, light_tree) == 0, HK_E_HIP, "device build of the light tree failed: %s", hipGetErrorString(hipGetLastError()));
  }
  c->mirrors_stale = true;
  c->wide_tlas_dirty = true;
  c->device_tree_builds += 1;
  return HK_OK;
}
// Test hook: the instance tree (ordering 0) and the light tree as the device holds them, converted back to the reference layout
// (navigators that took over their single leaf's role - fold_leaf_navigators - point at the leaf again)
int hk_debug_read_trees(hk_ctx* c, HkNode* tlas, uint32_t tlas_cap, HkNode* light, uint32_t light_cap) {
  HK_REQUIRE(c && (tlas || !tlas_cap) && (light || !light_cap), HK_E_INVALID, "NULL argument");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = flush_deform(c))) return rc;
  if ((rc = sync_all(c))) return rc;
  const uint32_t nt = (uint32_t)c->instance_nodes.size(), nl = (uint32_t)c->emissive_nodes.size();
  HK_REQUIRE(tlas_cap >= nt && light_cap >= nl, HK_E_INVALID, "need room for %u + %u nodes", nt, nl);
  const uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  auto convert = [](const std::vector<float4>& lo, const std::vector<float4>& hi, HkNode* out) {
    const uint32_t n = (uint32_t)lo.size();
    auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    for (uint32_t k = 0; k < n; ++k) {
      out[k].min[0] = lo[k].x; out[k].min[1] = lo[k].y; out[k].min[2] = lo[k].z;
      out[k].max[0] = hi[k].x; out[k].max[1] = hi[k].y; out[k].max[2] = hi[k].z;
      out[k].entry_index = bits(lo[k].w);
      out[k].exit_index = bits(hi[k].w);
    }
    for (uint32_t k = 0; k + 1 < n; ++k)
      if (out[k].entry_index >= HK_BVH_LEAF_FLAG && out[k + 1].entry_index == out[k].entry_index && out[k + 1].exit_index == out[k].exit_index) out[k].entry_index = k + 1;
  };
  if (nt) {
    std::vector<float4> both(2 * (size_t)nt), lo(nt), hi(nt);
    HK_HIP(hipMemcpy(both.data(), base + c->dyn_off.tlas, both.size() * 16, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < nt; ++k) { lo[k] = both[2 * k]; hi[k] = both[2 * k + 1]; }
    convert(lo, hi, tlas);
  }
  if (nl) {
    std::vector<float4> lo(nl), hi(nl);
    HK_HIP(hipMemcpy(lo.data(), base + c->dyn_off.light_lo, (size_t)nl * 16, hipMemcpyDeviceToHost));
    HK_HIP(hipMemcpy(hi.data(), base + c->dyn_off.light_hi, (size_t)nl * 16, hipMemcpyDeviceToHost));
    convert(lo, hi, light);
  }
  return HK_OK;
}

// `commit`: advance the builder's previous-transform bookkeeping (once per update, whichever context sees it last)
static int refit_impl(hk_ctx* c, hk_scene_builder* b, uint32_t* moved_out, bool commit) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  const uint32_t ni = (uint32_t)c->instances.size();
  HK_REQUIRE(builder_instance_count(b) == ni, HK_E_INVALID, "the builder has %u instances, the uploaded scene %u: instances were added or removed (use hk_upload_scene_instances)",
             builder_instance_count(b), ni);
  // which instances moved since the pose the device holds; their new host-side records (the reference's per-instance work,
  // instance.rs:286-325, kept in step so that a later host-side rebuild starts from the right poses)
  std::vector<uint32_t> moved;
  std::vector<hkd::RefitUpdate> records;
  for (uint32_t i = 0; i < ni; ++i) {
    InstanceDecl d;
    HK_REQUIRE(builder_instance_decl(b, i, &d), HK_E_NOT_READY, "the builder has unfinished mesh changes (hk_scene_builder_finish + hk_upload_scene first)");
    HkInstance& in = c->instances[i];
    HK_REQUIRE(d.material == in.material && memcmp(&d.mesh, &in.mesh, sizeof(HkMeshIndex)) == 0, HK_E_INVALID,
               "instance %u changed its mesh or material (use hk_upload_scene_instances)", i);
    if (memcmp(d.transform, in.model, 64) == 0) continue;
    float mn[3], mx[3], itm[16];
    HK_REQUIRE(instance_world_record(d.transform, d.aabb_center, d.aabb_half, mn, mx, itm), HK_E_INVALID, "singular transform of instance %u", i);
    hkd::RefitUpdate u;
    u.instance = i;
    u.moved = 1u;
    memcpy(u.model, d.transform, 64);
    memcpy(u.aabb_center, d.aabb_center, 12);
    memcpy(u.aabb_half, d.aabb_half, 12);
    records.push_back(u);
    moved.push_back(i);
  }
  if (moved_out) *moved_out = (uint32_t)moved.size();
  // hk_update_materials switched an emitter in this frame and took these poses along (hk_update_scene_instances' path): nothing is left
  // to do - the instances that moved in it keep their `moved` flag until the next frame's refit
  // (rf_motion_taken: set by update_materials_impl's case B, cleared by the next frame - context.hip ready())
  if (moved.empty() && c->rf_motion_taken) return HK_OK;
  if ((rc = prepare_refit(c))) return rc;
  {  // instances that moved in the previous update and rest now: their `moved` flag goes (previous model = model)
    std::vector<uint8_t> now(ni, 0);
    for (uint32_t i : moved) now[i] = 1;
    for (uint32_t i : c->rf_last_moved)
      if (!now[i]) {
        hkd::RefitUpdate u{};
        u.instance = i;
        u.moved = 0u;
        records.push_back(u);
      }
  }
  if (records.empty()) {
    if (commit) builder_commit_transforms(b);
    return HK_OK;
  }
  // the records of moved emitters first (k_refit_emitters runs one wave per such record and on no other)
  uint32_t n_emitter_updates = 0, emitter_triangles = 0;
  {
    std::vector<uint8_t> is_emitter(ni, 0);
    for (const HkEmissive& e : c->emissives)
      if (e.instance < ni) is_emitter[e.instance] = 1;
    auto mid = std::stable_partition(records.begin(), records.end(), [&](const hkd::RefitUpdate& u) { return u.moved && is_emitter[u.instance]; });
    n_emitter_updates = (uint32_t)(mid - records.begin());
    for (uint32_t k = 0; k < n_emitter_updates; ++k)
      emitter_triangles = std::max(emitter_triangles, (c->instances[records[k].instance].mesh.node_count + 2u) / 3u);  // a BLAS over n triangles: 3n - 2 nodes
  }
  // pinned update records, double-buffered against the kernel that reads them
  const int k = c->rf_k;
  c->rf_k ^= 1;
  if (c->rf_pending[k]) {
    HK_HIP(hipEventSynchronize(c->rf_done[k]));
    c->rf_pending[k] = false;
  }
  if (c->rf_updates_cap[k] < records.size()) {
    if (c->rf_updates[k]) (void)hipHostFree(c->rf_updates[k]);
    c->rf_updates[k] = nullptr;
    c->rf_updates_cap[k] = 0;
    const size_t cap = records.size() + records.size() / 2 + 16;
    HK_HIP(hipHostMalloc((void**)&c->rf_updates[k], cap * sizeof(hkd::RefitUpdate), hipHostMallocDefault));
    c->rf_updates_cap[k] = cap;
  }
  if (!c->rf_done[k]) HK_HIP(hipEventCreateWithFlags(&c->rf_done[k], hipEventDisableTiming));
  memcpy(c->rf_updates[k], records.data(), records.size() * sizeof(hkd::RefitUpdate));
  // frames in flight keep reading the slot they were enqueued with: refit a copy in the spare slot (two-slot scenes), or in
  // place behind everything enqueued so far (scenes small enough for the LDS copy have one slot)
  if ((rc = begin_device_update(c))) return rc;
  const hkd::RefitScene r = refit_scene(c);
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  launch_refit(c->stream, r, c->rf_updates[k], (uint32_t)records.size(), n_emitter_updates, emitter_triangles, nullptr, (float4*)(base + c->dyn_off.tlas), (uint32_t)c->instance_nodes.size(),
               c->threaded ? 8u : 1u, (float4*)(base + c->dyn_off.light_lo), (float4*)(base + c->dyn_off.light_hi), (uint32_t)c->emissive_nodes.size());
  HK_HIP(hipGetLastError());
  // a deformed mesh's box is the device's, not the builder's: its instances' boxes, emitters and both trees once more from it
  if (c->meshes_deformed && (rc = repropagate_deformed(c))) return rc;
  HK_HIP(hipEventRecord(c->rf_done[k], c->stream));
  c->rf_pending[k] = true;
  // the update is enqueued: now the host mirrors of the moved instances follow (an error above leaves host and device agreeing)
  for (const hkd::RefitUpdate& u : records) {
    if (!u.moved) continue;
    HkInstance& in = c->instances[u.instance];
    if (c->prev_models.size() != 16 * (size_t)ni) {
      c->prev_models.resize(16 * (size_t)ni);
      for (uint32_t j = 0; j < ni; ++j) memcpy(&c->prev_models[16 * (size_t)j], c->instances[j].model, 64);
    }
    memcpy(&c->prev_models[16 * (size_t)u.instance], in.model, 64);
    memcpy(in.model, u.model, 64);
    (void)instance_world_record(u.model, u.aabb_center, u.aabb_half, in.min, in.max, in.inverse_transpose_model);
  }
  for (const hkd::RefitUpdate& u : records)
    if (!u.moved && c->prev_models.size() == 16 * (size_t)ni) memcpy(&c->prev_models[16 * (size_t)u.instance], c->instances[u.instance].model, 64);
  update_shared_transform(c);  // (a scene in one slot is refit in place: nothing else looks at the new poses before the next frame)
  c->d_prev_models = c->rf_prev_models;
  c->rf_last_moved = moved;
  c->mirrors_stale = true;
  c->wide_tlas_dirty = true;
  c->device_refits += 1;
  if (commit) builder_commit_transforms(b);
  return HK_OK;
}
int hk_refit_scene_instances(hk_ctx* c, hk_scene_builder* b, uint32_t* moved_out) { return refit_impl(c, b, moved_out, true); }}  // extern "C"
int hk::refit_instances_impl(hk_ctx* c, hk_scene_builder* b, uint32_t* moved, bool commit) { return refit_impl(c, b, moved, commit); }

// ---- material edits on the device (hikari_hip.h hk_update_materials; kernels in kernels_scene.hip) ---------------------------------
// The reference re-runs prepare_instances when a material changes (instance.rs:352-437).  What a change of VALUES touches is the
// material record and, for emitters, the radius (instance.rs:382,409) with the light tree's leaf boxes: a few records through pinned
// memory, one kernel over the emitters concerned and the light-tree refit (case A).  Only an emitter switched on or off changes the
// layout of the region: that edit takes the instance-set path, hk_update_scene_instances (case B).
// The instance-level records of a builder finished with stand-in trees, then both trees built on the device - what every band but the
// one that finished the builder does in hk_multi_update_scene_instances / hk_multi_update_materials.  Stand-in trees never stay
// (hk_update_scene_instances): if the upload went through and the build did not, the next use lays the region out again.
int hk::upload_instances_and_build_trees(hk_ctx* c, const hk_scene_builder* b, uint32_t tree_mode) {
  uint32_t ni = 0;
  const HkInstance* inst = nullptr;
  int rc;
  if ((rc = hk_scene_builder_instances(b, &inst, &ni))) return rc;
  const size_t n_materials = c->materials.size();
  if ((rc = take_appended_materials(c, b))) return rc;
  if ((rc = upload_scene_instances_unchecked(c, b))) {  // (its refusals write nothing: the material mirror is what it was)
    c->materials.resize(n_materials);
    return rc;
  }
  if (ni >= 2 && (rc = hk_rebuild_scene_trees(c, tree_mode))) c->dynamic_dirty = true;
  return rc;
}
int hk::update_materials_impl(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode, uint32_t* changed_out, bool finish) {
  HK_REQUIRE(c && b, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(tree_mode == HK_TREE_SAH || tree_mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", tree_mode);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  {
    InstanceDecl d;
    HK_REQUIRE(builder_instance_count(b) == 0u || builder_instance_decl(b, 0u, &d), HK_E_NOT_READY,
               "the builder has unfinished mesh changes (hk_scene_builder_finish + hk_upload_scene first)");
  }
  HK_NO_PENDING_MESHES(b);
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  const HkMaterial* mats = nullptr;
  uint32_t nm = 0;
  builder_materials(b, &mats, &nm);
  HK_REQUIRE(nm == c->materials.size(), HK_E_INVALID, "the builder has %u materials, the uploaded scene %zu: materials were added (use hk_upload_scene)", nm, c->materials.size());
  // which records differ from the ones the device holds; 1: values, 2: the emissive colour too (bit for bit)
  std::vector<uint8_t> differs(nm, 0);
  std::vector<uint32_t> ids;
  const uint32_t n_tex = (uint32_t)c->textures.size();
  for (uint32_t i = 0; i < nm; ++i) {
    if (memcmp(&mats[i], &c->materials[i], sizeof(HkMaterial)) == 0) continue;
    for (uint32_t id : {mats[i].base_color_texture, mats[i].emissive_texture, mats[i].metallic_roughness_texture, mats[i].occlusion_texture})
      HK_REQUIRE(id == HK_NO_TEXTURE || id < n_tex, HK_E_INVALID, "material %u references texture %u but only %u textures are uploaded", i, id, n_tex);
    differs[i] = memcmp(mats[i].emissive, c->materials[i].emissive, 16) == 0 ? 1 : 2;
    ids.push_back(i);
  }
  if (changed_out) *changed_out = (uint32_t)ids.size();
  if (ids.empty()) return HK_OK;
  c->scene_epoch += 1;   // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining - a refusal above leaves it alone)
  // case B: an instance starts or stops emitting - the emitter list, the alias tables and the light tree change size - or the builder's
  // instance set is not the uploaded one (instances added or removed, another mesh or material for one: what the refit refuses): case A
  // works from the context's instance records and would drop such an edit, the instance-set path takes it along
  const uint32_t ni = (uint32_t)c->instances.size();
  bool set_changes = builder_instance_count(b) != ni;
  for (uint32_t i = 0; i < ni && !set_changes; ++i) {
    const HkInstance& in = c->instances[i];
    InstanceDecl d;
    set_changes = !builder_instance_decl(b, i, &d) || d.material != in.material || memcmp(&d.mesh, &in.mesh, sizeof(HkMeshIndex)) != 0 ||
                  (differs[in.material] == 2 && material_emits(mats[in.material]) != material_emits(c->materials[in.material]));
  }
  if (set_changes) {
    // (refusals - a mesh deformed on the device - come from the path taken, before it writes anything: the old materials then return)
    std::vector<HkMaterial> old(mats, mats + nm);
    c->materials.swap(old);
    // a later band of hk_multi_update_materials finds the builder finished already, with stand-in trees
    rc = finish ? hk_update_scene_instances(c, b, tree_mode) : upload_instances_and_build_trees(c, b, tree_mode);
    if (rc) c->materials.swap(old);
    else c->rf_motion_taken = true;   // (hk_context.hpp: poses set on the builder travelled with this update)
    return rc;
  }
  // case A.  The device's current boxes first (a mesh deformed since the last frame), as hk_rebuild_scene_trees does
  if ((rc = flush_deform(c))) return rc;
  std::vector<uint32_t> emitters;  // whose instance uses a material with a new emissive colour
  for (size_t e = 0; e < c->emissives.size(); ++e)
    if (differs[c->instances[c->emissives[e].instance].material] == 2) emitters.push_back((uint32_t)e);
  if (!emitters.empty() && (rc = prepare_refit(c))) return rc;
  // pinned records - the materials, then the emitter ids - double-buffered against the kernels that read them
  const size_t rec_bytes = ids.size() * sizeof(hkd::MaterialUpdate), bytes = rec_bytes + emitters.size() * 4;
  const int k = c->mt_k;
  c->mt_k ^= 1;
  if (c->mt_pending[k]) {
    HK_HIP(hipEventSynchronize(c->mt_done[k]));
    c->mt_pending[k] = false;
  }
  if (c->mt_updates_cap[k] < bytes) {
    if (c->mt_updates[k]) (void)hipHostFree(c->mt_updates[k]);
    c->mt_updates[k] = nullptr;
    c->mt_updates_cap[k] = 0;
    const size_t cap = bytes + bytes / 2 + 256;
    HK_HIP(hipHostMalloc((void**)&c->mt_updates[k], cap, hipHostMallocDefault));
    c->mt_updates_cap[k] = cap;
  }
  if (!c->mt_done[k]) HK_HIP(hipEventCreateWithFlags(&c->mt_done[k], hipEventDisableTiming));
  hkd::MaterialUpdate* records = (hkd::MaterialUpdate*)c->mt_updates[k];
  for (size_t u = 0; u < ids.size(); ++u) {
    records[u].material = ids[u];
    records[u].pad[0] = records[u].pad[1] = records[u].pad[2] = 0u;
    material_rows(mats[ids[u]], records[u].rows);
  }
  uint32_t* emitter_ids = (uint32_t*)(c->mt_updates[k] + rec_bytes);
  if (!emitters.empty()) memcpy(emitter_ids, emitters.data(), emitters.size() * 4);
  // frames in flight keep reading the slot they were enqueued with (begin_device_update)
  if ((rc = begin_device_update(c))) return rc;
  const hkd::RefitScene r = refit_scene(c);
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  launch_material_update(c->stream, r, (float4*)(base + c->dyn_off.materials), records, (uint32_t)ids.size(), emitter_ids, (uint32_t)emitters.size(),
                         (float4*)(base + c->dyn_off.light_lo), (float4*)(base + c->dyn_off.light_hi), (uint32_t)c->emissive_nodes.size());
  HK_HIP(hipGetLastError());
  HK_HIP(hipEventRecord(c->mt_done[k], c->stream));
  c->mt_pending[k] = true;
  // the update is enqueued: now the host mirror follows (an error above leaves host and device agreeing)
  for (uint32_t e : emitters) memcpy(c->emissives[e].emissive, mats[c->instances[c->emissives[e].instance].material].emissive, 16);
  c->materials.assign(mats, mats + nm);
  if (!emitters.empty()) c->mirrors_stale = true;  // (radius and light-tree boxes are the device's from here on)
  return HK_OK;
}
extern "C" int hk_update_materials(hk_ctx* c, hk_scene_builder* b, uint32_t tree_mode, uint32_t* changed) { return hk::update_materials_impl(c, b, tree_mode, changed, true); }
