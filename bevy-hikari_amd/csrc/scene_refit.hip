// scene_refit.hip - instance motion and instance-set changes on the device (kernels in kernels_scene.hip, tree builds in kernels_tree.hip): the
// reference re-runs prepare_instances on the host for ANY instance change (instance.rs:352-437); here moved instances are refit,
// both trees rebuilt (the reference's SAH tree or an LBVH) and instance-set edits laid out without the host's two tree builds.
#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

namespace {
// what the calls that diff or lay out from the host's pose mirrors answer after hk_set_instance_transforms_device (hk_context.hpp poses_on_device)
const char* const kPosesOnDevice =
    "the instances' poses were last set from device memory (hk_set_instance_transforms_device): read them back (hk_read_instance_transforms), put them on "
    "the builder and upload the instances again (hk_upload_scene_instances) first";
}  // namespace

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
  HK_REQUIRE(!c->poses_on_device, HK_E_NOT_READY, "%s", kPosesOnDevice);
  HK_NO_PENDING_MESHES(b);  // (before the builder is finished: a refusal changes nothing)
  int rc;
  const bool trace = c->trace_update;
  const double t0 = now_ms();
  if ((rc = hk_scene_builder_finish_instances(b))) return rc;
  const double t1 = now_ms();
  const size_t n_materials = c->materials.size();
  if ((rc = take_appended_materials(c, b))) return rc;  // (a spawned object is a mesh, a material and an instance; refused ids write nothing)
  if ((rc = upload_scene_instances_unchecked(c, b))) {  // (refused: the material mirror is what it was)
    c->materials.resize(n_materials);
    return rc;
  }
  const double t2 = now_ms();
  uint32_t ni = 0;
  const HkInstance* inst = nullptr;
  if ((rc = hk_scene_builder_instances(b, &inst, &ni))) return rc;
  c->trees_pending_on_device = ni >= 2;
  rc = finalize_scene(c);
  c->trees_pending_on_device = false;
  const double t3 = now_ms();
  if (!rc && ni >= 2) rc = hk_rebuild_scene_trees(c, tree_mode);  // (a tree of one leaf is what the host just laid out)
  // the region just uploaded carries stand-in trees with orderings 1..7 left zero (the device build was to overwrite
  // them in stream order).  If that build did not get enqueued, a threaded walk over zero nodes would never leave node 0: the
  // next use of the scene lays the region out again, from the host's (valid) stand-in trees, all orderings threaded.
  if (rc) c->dynamic_dirty = true;
  if (trace) fprintf(stderr, "hk_update_scene_instances: finish_instances %.2f ms, mirrors %.2f ms, layout + upload %.2f ms, device build enqueue %.2f ms\n", t1 - t0, t2 - t1, t3 - t2, now_ms() - t3);
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
  for (void* q : {(void*)c->pd_boxes, (void*)c->pd_all, (void*)c->pd_records})
    if (q) (void)hipFree(q);
  c->pd_boxes = nullptr; c->pd_all = nullptr; c->pd_records = nullptr;
  c->pd_cap = 0;
  c->pd_all_ready = false;
  c->pd_boxes_host.clear();
  for (hipEvent_t* e : {&c->pd_src_ready, &c->pd_src_read}) {
    if (*e) (void)hipEventDestroy(*e);
    *e = nullptr;
  }
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
// room in the refit's side arrays for `ni` instances and `na` alias entries (waits only where they grow)
int reserve_refit(hk_ctx* c, size_t ni, size_t na) {
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
  return HK_OK;
}
// side arrays of the refit, (re)filled from the scene as the host last laid it out: world AABB per instance from the TLAS
// leaves, emitter of an instance, previous models
int prepare_refit(hk_ctx* c) {
  if (c->rf_ready) return HK_OK;
  const size_t ni = c->instances.size(), na = c->alias_table.size();
  const int rc_reserve = reserve_refit(c, ni, na);
  if (rc_reserve) return rc_reserve;
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
    repoint_scene(c);
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
  if ((rc = reserve_tree_scratch(c, ni, ne))) return rc;
  if ((rc = begin_device_update(c))) return rc;
  return build_trees_in_slot(c, mode);
}
}  // extern "C"
// the scratch of the two tree builds (waits only where it grows)
int hk::reserve_tree_scratch(hk_ctx* c, uint32_t ni, uint32_t ne) {
  int rc;
  const size_t need = std::max(lbvh_scratch_bytes(ni), lbvh_scratch_bytes(std::max(ne, 1u)));
  if (need > c->lbvh_scratch_cap) {
    if ((rc = sync_all(c))) return rc;
    if (c->lbvh_scratch) (void)hipFree(c->lbvh_scratch);
    c->lbvh_scratch = nullptr;
    c->lbvh_scratch_cap = 0;
    HK_HIP(hipMalloc(&c->lbvh_scratch, need + need / 4));
    c->lbvh_scratch_cap = need + need / 4;
  }
  return HK_OK;
}
int hk::build_trees_in_slot(hk_ctx* c, uint32_t mode) {
  const uint32_t ni = (uint32_t)c->instances.size(), ne = (uint32_t)c->emissives.size();
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
extern "C" {
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
  HK_REQUIRE(!c->poses_on_device, HK_E_NOT_READY, "%s", kPosesOnDevice);  // (the diff below would be against poses the device no longer holds)
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
int hk_refit_scene_instances(hk_ctx* c, hk_scene_builder* b, uint32_t* moved_out) { return refit_impl(c, b, moved_out, true); }

// ---- instance poses from device memory (hikari_hip.h hk_set_instance_transforms_device; kernels k_pose_begin / k_pose_records) --------
// What refit_impl does with poses the host never sees: the diff against the device's models, the records and the `moved` rule move into
// two kernels, k_refit_instances / k_refit_emitters and the tree refits follow unchanged.  The host keeps what it still knows - which
// instances emit, the builder's mesh boxes (a device plane, copied only when they changed) - and stops trusting its pose mirrors.
}  // extern "C"
namespace {
// memory the context's device can read - its own, or host memory mapped for it - `extent` bytes from `p` on inside its allocation
// (mesh_deform.hip check_source states the rule for hk_deform_meshes_device)
int check_pose_memory(hk_ctx* c, const char* what, const void* p, size_t extent) {
  HK_REQUIRE(((uintptr_t)p & 3u) == 0, HK_E_INVALID, "%s at %p is not aligned to 4 bytes", what, p);
  hipPointerAttribute_t a{};
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) (void)hipGetLastError();
  HK_REQUIRE(e == hipSuccess && ((a.type == hipMemoryTypeDevice && a.device == c->device) || a.type == hipMemoryTypeHost), HK_E_INVALID,
             "%s at %p is neither memory of device %d nor host memory the device can access", what, p, c->device);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {  // (mapped host memory may have no range to ask for)
    (void)hipGetLastError();
    HK_REQUIRE(a.type == hipMemoryTypeHost, HK_E_INVALID, "%s at %p: the extent of its allocation is unknown", what, p);
    return HK_OK;
  }
  HK_REQUIRE((const uint8_t*)p + extent <= (const uint8_t*)base + size, HK_E_INVALID, "%s reaches %zu bytes beyond its allocation", what,
             (size_t)(((const uint8_t*)p + extent) - ((const uint8_t*)base + size)));
  return HK_OK;
}
}  // namespace
extern "C" {

int hk_set_instance_transforms_device(hk_ctx* c, hk_scene_builder* b, const uint32_t* ids, uint32_t n, const void* d_models, uint32_t stride_bytes, void* producer_stream,
                                      uint32_t* d_status) {
  HK_REQUIRE(c && b && d_models, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(!(ids && n == 0), HK_E_INVALID, "instance ids given for no instance");
  HK_REQUIRE(stride_bytes >= 64 && stride_bytes % 4 == 0, HK_E_INVALID, "a stride of %u bytes: a pose is 64 bytes, and strides are multiples of 4", stride_bytes);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_HIP(hipSetDevice(c->device));
  const uint32_t ni = (uint32_t)c->instances.size();
  int rc;
  // ---- the whole call is validated before anything is enqueued or written
  HK_REQUIRE(n <= ni, HK_E_INVALID, "%u poses for a scene of %u instances", n, ni);
  std::vector<uint8_t> is_emitter(ni, 0);
  for (const HkEmissive& e : c->emissives)
    if (e.instance < ni) is_emitter[e.instance] = 1;
  const bool all = !ids && n == ni;  // every instance named, in order: the record order is cached on the device
  std::vector<uint2> named;          // (instance, index of its pose in the caller's memory), emitters first
  uint32_t n_emitter_updates = 0, emitter_triangles = 0;
  if (!all) {
    std::vector<uint8_t> seen(ni, 0);
    named.resize(n);
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t id = ids ? ids[k] : k;
      HK_REQUIRE(id < ni, HK_E_INVALID, "instance id %u (entry %u) of a scene of %u instances", id, k, ni);
      HK_REQUIRE(!seen[id], HK_E_INVALID, "instance %u is named twice (entry %u)", id, k);
      seen[id] = 1;
      if (is_emitter[id]) ++n_emitter_updates;
    }
    size_t front = 0, back = n_emitter_updates;
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t id = ids ? ids[k] : k;
      named[is_emitter[id] ? front++ : back++] = make_uint2(id, k);
      if (is_emitter[id]) emitter_triangles = std::max(emitter_triangles, (c->instances[id].mesh.node_count + 2u) / 3u);  // a BLAS over n triangles: 3n - 2 nodes
    }
  }
  if (n && (rc = check_pose_memory(c, "the pose array", d_models, (size_t)(n - 1) * stride_bytes + 64))) return rc;
  if (d_status && (rc = check_pose_memory(c, "the status word", d_status, 4))) return rc;
  HK_REQUIRE(builder_instance_count(b) == ni, HK_E_INVALID, "the builder has %u instances, the uploaded scene %u: instances were added or removed (use hk_upload_scene_instances)",
             builder_instance_count(b), ni);
  bool boxes_changed = !c->pd_boxes || c->pd_boxes_host.size() != 8 * (size_t)ni;
  for (uint32_t i = 0; i < ni; ++i) {
    InstanceDecl d;
    HK_REQUIRE(builder_instance_decl(b, i, &d), HK_E_NOT_READY, "the builder has unfinished mesh changes (hk_scene_builder_finish + hk_upload_scene first)");
    const HkInstance& in = c->instances[i];
    HK_REQUIRE(d.material == in.material && memcmp(&d.mesh, &in.mesh, sizeof(HkMeshIndex)) == 0, HK_E_INVALID,
               "instance %u changed its mesh or material (use hk_upload_scene_instances)", i);
    if (!boxes_changed) {
      const float* h = &c->pd_boxes_host[8 * (size_t)i];
      boxes_changed = memcmp(h, d.aabb_center, 12) != 0 || memcmp(h + 4, d.aabb_half, 12) != 0;
    }
  }
  // ---- the scene as laid out, the refit's side arrays, the planes of this path (waits only where something is missing or grows)
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = prepare_refit(c))) return rc;
  if (ni > c->pd_cap) {
    if ((rc = sync_all(c))) return rc;
    for (void* q : {(void*)c->pd_boxes, (void*)c->pd_all, (void*)c->pd_records})
      if (q) (void)hipFree(q);
    c->pd_boxes = nullptr; c->pd_all = nullptr; c->pd_records = nullptr;
    c->pd_cap = 0;
    c->pd_all_ready = false;
    const size_t cap = (size_t)ni + ni / 4;
    HK_HIP(hipMalloc((void**)&c->pd_boxes, cap * 32));
    HK_HIP(hipMalloc((void**)&c->pd_all, cap * sizeof(uint2)));
    HK_HIP(hipMalloc((void**)&c->pd_records, cap * sizeof(hkd::RefitUpdate)));
    c->pd_cap = cap;
    boxes_changed = true;
  }
  c->last_pose[1] = boxes_changed ? 1u : 0u;
  if (boxes_changed) {  // the builder's mesh boxes (builder_instance_decl, as refit_impl takes them): once per instance list, not per call
    std::vector<float>& h = c->pd_boxes_host;
    h.assign(8 * (size_t)ni, 0.0f);
    for (uint32_t i = 0; i < ni; ++i) {
      InstanceDecl d;
      (void)builder_instance_decl(b, i, &d);
      memcpy(&h[8 * (size_t)i], d.aabb_center, 12);
      memcpy(&h[8 * (size_t)i + 4], d.aabb_half, 12);
    }
    HK_HIP(hipMemcpyAsync(c->pd_boxes, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->stream));  // (behind the last call's kernels, which read the plane)
    HK_HIP(hipStreamSynchronize(c->stream));
  }
  if (all && (!c->pd_all_ready || c->pd_all_generation != c->instances_generation)) {
    std::vector<uint2> order(ni);
    size_t front = 0, back = (size_t)std::count(is_emitter.begin(), is_emitter.end(), (uint8_t)1);
    uint32_t triangles = 0;
    for (uint32_t i = 0; i < ni; ++i) {
      order[is_emitter[i] ? front++ : back++] = make_uint2(i, i);
      if (is_emitter[i]) triangles = std::max(triangles, (c->instances[i].mesh.node_count + 2u) / 3u);
    }
    HK_HIP(hipMemcpyAsync(c->pd_all, order.data(), order.size() * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
    HK_HIP(hipStreamSynchronize(c->stream));  // (`order` is a local; once per instance list)
    c->pd_all_emitters = (uint32_t)front;
    c->pd_all_emitter_triangles = triangles;
    c->pd_all_generation = c->instances_generation;
    c->pd_all_ready = true;
  }
  const uint2* d_named = c->pd_all;
  int k = -1;
  if (all) {
    n_emitter_updates = c->pd_all_emitters;
    emitter_triangles = c->pd_all_emitter_triangles;
  } else if (n) {  // the call's own list, read by the kernel from a pinned block of the pool
    uint8_t* st = nullptr;
    if ((rc = stage(c, named.size() * sizeof(uint2), &st, &k))) return rc;
    memcpy(st, named.data(), named.size() * sizeof(uint2));
    d_named = (const uint2*)st;
  }
  hipStream_t producer = n ? (hipStream_t)producer_stream : nullptr;
  if (producer)
    for (hipEvent_t* e : {&c->pd_src_ready, &c->pd_src_read})
      if (!*e) HK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  // ---- enqueue.  Frames in flight keep reading the slot they were enqueued with (begin_device_update)
  if ((rc = begin_device_update(c))) return rc;
  if (producer) {  // what the producer has enqueued on the poses so far comes first; it may write them again once k_pose_records has read them
    HK_HIP(hipEventRecord(c->pd_src_ready, producer));
    HK_HIP(hipStreamWaitEvent(c->stream, c->pd_src_ready, 0));
  }
  c->scene_epoch += 1;   // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining - a refusal above leaves it alone)
  const hkd::RefitScene r = refit_scene(c);
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  const uint32_t tlas_count = (uint32_t)c->instance_nodes.size(), light_count = (uint32_t)c->emissive_nodes.size();
  uint32_t launches = launch_pose_records(c->stream, r, ni, d_named, n, d_models, stride_bytes, c->pd_boxes, c->pd_records, d_status, producer ? c->pd_src_read : nullptr);
  HK_HIP(hipGetLastError());
  if (producer) HK_HIP(hipStreamWaitEvent(producer, c->pd_src_read, 0));
  launch_refit(c->stream, r, c->pd_records, n, n_emitter_updates, emitter_triangles, nullptr, (float4*)(base + c->dyn_off.tlas), tlas_count, c->threaded ? 8u : 1u,
               (float4*)(base + c->dyn_off.light_lo), (float4*)(base + c->dyn_off.light_hi), light_count);
  HK_HIP(hipGetLastError());
  launches += (n ? 1u : 0u) + (n && n_emitter_updates ? 1u : 0u) + (tlas_count ? 1u : 0u) + (light_count ? 1u : 0u);
  if (k >= 0) {
    hk_ctx::DeformStage& st = c->df_stage[(size_t)k];
    HK_HIP(hipEventRecord(st.done, c->stream));
    st.pending = true;
  }
  // a deformed mesh's box is the device's, not the builder's: its instances' boxes, emitters and both trees once more from it
  if (c->meshes_deformed && (rc = repropagate_deformed(c))) return rc;
  // the update is enqueued: from here on the host's pose mirrors describe the scene as it was (the builder was not told either)
  c->poses_on_device = true;
  update_shared_transform(c);
  c->d_prev_models = c->rf_prev_models;
  c->rf_last_moved.clear();  // (the flags are the device's: k_pose_begin clears what an earlier update left)
  c->mirrors_stale = true;
  c->wide_tlas_dirty = true;
  c->device_refits += 1;
  c->last_pose[0] = launches;
  return HK_OK;
}

// The way back: the models the device holds, in the slot the next frame would read.  Waits for the context's streams.
int hk_read_instance_transforms(hk_ctx* c, float* models, uint32_t n) {
  HK_REQUIRE(c && models, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_REQUIRE(n == c->instances.size(), HK_E_INVALID, "room for %u poses, the scene has %zu instances", n, c->instances.size());
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = sync_all(c))) return rc;
  std::vector<DInstance> records(n);
  HK_HIP(hipMemcpy(records.data(), c->scene_mem + (size_t)c->slot * c->dyn_capacity + c->dyn_off.instances, (size_t)n * sizeof(DInstance), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    const float4 col[4] = {records[i].m0, records[i].m1, records[i].m2, records[i].m3};
    memcpy(models + 16 * (size_t)i, col, 64);
    memcpy(c->instances[i].model, col, 64);  // (the flag stays: boxes, inverses and previous models are still the device's alone)
  }
  return HK_OK;
}
// Test hook (hikari_hip_debug.h)
int hk_debug_last_pose(hk_ctx* c, uint32_t out[2]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  out[0] = c->last_pose[0];
  out[1] = c->last_pose[1];
  return HK_OK;
}
}  // extern "C"
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
    HK_REQUIRE(!c->poses_on_device, HK_E_NOT_READY, "%s", kPosesOnDevice);  // (this case lays the instances out from the builder's poses)
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
