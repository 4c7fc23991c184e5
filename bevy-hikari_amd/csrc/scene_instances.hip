// scene_instances.hip - the instance set changed from DEVICE state (hikari_hip.h hk_change_scene_instances; kernels in kernels_scene.hip;
// DESIGN 4 "Instance set changes from device state").  hk_update_scene_instances lays the instance level out from the host's mirrors and
// is refused once they are stale - after a mesh deformation, after poses set from device memory.  Only VALUES are stale then: the layout
// of the level - counts, offsets, which instance emits, the length of every alias slice - follows from topology and materials, which the
// host knows in every state.  So the host lays the new level out as ever, stale numbers and all, into the spare slot, and the device
// writes its own values over them: the survivors' poses from the old slot, every world box from the current mesh boxes, every emitter
// record and alias slice from the current triangles, then both trees.
#include <cmath>

#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

namespace {
bool finite16(const float* m) {
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(m[k])) return false;
  return true;
}
}  // namespace

int hk::check_appended_materials(const hk_ctx* c, const hk_scene_builder* b) {
  const HkMaterial* mats = nullptr;
  uint32_t nm = 0;
  builder_materials(b, &mats, &nm);
  const uint32_t n_tex = (uint32_t)c->textures.size();
  for (uint32_t i = (uint32_t)c->materials.size(); i < nm; ++i)
    for (uint32_t id : {mats[i].base_color_texture, mats[i].emissive_texture, mats[i].metallic_roughness_texture, mats[i].occlusion_texture})
      HK_REQUIRE(id == HK_NO_TEXTURE || id < n_tex, HK_E_INVALID, "material %u references texture %u but only %u textures are uploaded", i, id, n_tex);
  return HK_OK;
}
// hk_update_scene_instances: materials appended on the builder travel with that call's layout (changed VALUES: hk_update_materials)
int hk::take_appended_materials(hk_ctx* c, const hk_scene_builder* b) {
  const HkMaterial* mats = nullptr;
  uint32_t nm = 0;
  builder_materials(b, &mats, &nm);
  if (!c->have_materials || nm <= c->materials.size()) return HK_OK;
  const int rc = check_appended_materials(c, b);
  if (!rc) c->materials.insert(c->materials.end(), mats + c->materials.size(), mats + nm);
  return rc;
}

// `finish`: the builder is finished here (once per change, whichever context sees it first: hk_multi_change_scene_instances)
int hk::change_instances_impl(hk_ctx* c, hk_scene_builder* b, const uint32_t* origins, uint32_t n, uint32_t tree_mode, bool finish) {
  // ---- the whole call is validated before the builder is finished or anything is written
  HK_REQUIRE(c && b && origins, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(tree_mode == HK_TREE_SAH || tree_mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", tree_mode);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_NO_PENDING_MESHES(b);
  HK_REQUIRE(n == builder_instance_count(b), HK_E_INVALID, "%u origins for a builder of %u instances", n, builder_instance_count(b));
  HK_REQUIRE(n >= 1u, HK_E_INVALID, "a scene keeps at least one instance");
  const uint32_t n_old = (uint32_t)c->instances.size();
  const bool device_poses = c->poses_on_device;
  uint32_t n_carried = 0;
  {
    std::vector<uint8_t> seen(n_old, 0);
    for (uint32_t k = 0; k < n; ++k) {
      InstanceDecl d;
      HK_REQUIRE(builder_instance_decl(b, k, &d), HK_E_NOT_READY, "the builder has unfinished mesh changes (hk_add_meshes / hk_remove_meshes first)");
      const uint32_t o = origins[k];
      float mn[3], mx[3], itm[16];
      if (o == HK_INSTANCE_NEW) {
        HK_REQUIRE(finite16(d.transform) && instance_world_record(d.transform, d.aabb_center, d.aabb_half, mn, mx, itm), HK_E_INVALID,
                   "instance %u is new and its transform is singular or not finite", k);
        continue;
      }
      HK_REQUIRE(o < n_old, HK_E_INVALID, "origin %u of instance %u: the scene holds %u instances", o, k, n_old);
      HK_REQUIRE(!seen[o], HK_E_INVALID, "origin %u is named twice (instance %u)", o, k);
      seen[o] = 1;
      ++n_carried;
      HK_REQUIRE(memcmp(&d.mesh, &c->instances[o].mesh, sizeof(HkMeshIndex)) == 0, HK_E_INVALID, "instance %u is not an instance of the mesh its origin %u has", k, o);
      // (with the poses on the device the builder's transform of a survivor is not looked at)
      HK_REQUIRE(device_poses || (finite16(d.transform) && instance_world_record(d.transform, d.aabb_center, d.aabb_half, mn, mx, itm)), HK_E_INVALID,
                 "the transform of instance %u is singular or not finite", k);
    }
  }
  {
    const HkMaterial* mats = nullptr;
    uint32_t nm = 0;
    builder_materials(b, &mats, &nm);
    HK_REQUIRE(nm >= c->materials.size(), HK_E_INVALID, "the builder has %u materials, the uploaded scene %zu", nm, c->materials.size());
    if (const int bad = check_appended_materials(c, b)) return bad;
  }
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;  // (a pending layout first; refused as ever with stale mirrors - nothing changed)
  HK_REQUIRE(c->two_slots || (!c->mirrors_stale && !c->meshes_deformed), HK_E_NOT_READY,
             "the scene is walked from its LDS copy (one slot) and was last changed on the device: a new layout of it comes from the host's mirror (hk_upload_scene)");

  // ---- where hk_update_scene_instances is accepted the mirrors are the scene: its path, its bytes
  if (!c->meshes_deformed && !device_poses) {
    const uint8_t* const mem = c->scene_mem;
    rc = finish ? hk_update_scene_instances(c, b, tree_mode) : upload_instances_and_build_trees(c, b, tree_mode);
    if (rc) return rc;
    c->last_instance_change[0] = 0u;
    c->last_instance_change[1] = n_carried;
    c->last_instance_change[2] = n - n_carried;
    c->last_instance_change[3] = (c->scene_mem != mem ? 1u : 0u) | 2u;
    return HK_OK;
  }

  // ---- the device path.  A mesh range no instance has used yet is still in reference form (scene_layout.hip build_static_region): only a
  // host layout of the mesh level gives it its leaf boxes
  for (uint32_t k = 0; k < n; ++k) {
    InstanceDecl d;
    (void)builder_instance_decl(b, k, &d);
    HK_REQUIRE(d.mesh.node_count && (size_t)d.mesh.node_offset + d.mesh.node_count <= c->node_prim_offset.size() &&
                   c->node_prim_offset[d.mesh.node_offset] == (int64_t)d.mesh.primitive &&
                   c->node_prim_offset[d.mesh.node_offset + d.mesh.node_count - 1] == (int64_t)d.mesh.primitive,
               HK_E_NOT_READY, "instance %u names a mesh no instance had used when the mesh level was laid out: its tree has no leaf boxes yet (hk_upload_scene)", k);
  }
  if (finish && (rc = hk_scene_builder_finish_instances(b))) return rc;
  const HkNode *b_nodes, *b_enodes; const HkInstance* b_inst; const HkEmissive* b_em; const HkAliasEntry* b_alias; const float* b_prev;
  uint32_t ni, nin, ne, nen, nal, npm;
  if ((rc = hk_scene_builder_instances(b, &b_inst, &ni))) return rc;
  if ((rc = hk_scene_builder_instance_nodes(b, &b_nodes, &nin))) return rc;
  if ((rc = hk_scene_builder_emissives(b, &b_em, &ne))) return rc;
  if ((rc = hk_scene_builder_emissive_nodes(b, &b_enodes, &nen))) return rc;
  if ((rc = hk_scene_builder_alias_table(b, &b_alias, &nal))) return rc;
  if ((rc = hk_scene_builder_previous_transforms(b, &b_prev, &npm))) return rc;
  HK_REQUIRE(ni == n && nin == 3 * (size_t)n - 2 && (ne == 0 || nen == 3 * (size_t)ne - 2), HK_E_UNSUPPORTED,
             "the builder's trees are not in the flatten_custom layout of a binary tree (3n - 2 nodes)");

  // what the kernels read per instance, and what the emitters' launch is sized by
  std::vector<InstanceDerive> derive(n);
  uint32_t emitter_triangles = 0;
  for (uint32_t k = 0; k < n; ++k) {
    InstanceDecl d;
    (void)builder_instance_decl(b, k, &d);
    InstanceDerive& e = derive[k];
    e.origin = origins[k] == HK_INSTANCE_NEW ? HK_U32_MAX : origins[k];
    e.emitter = HK_U32_MAX;
    e.box = deformed_mesh_box(c, d.mesh);
    memcpy(e.aabb_center, d.aabb_center, 12);
    memcpy(e.aabb_half, d.aabb_half, 12);
    e.pad[0] = e.pad[1] = 0u;
  }
  for (uint32_t e = 0; e < ne; ++e) {
    HK_REQUIRE(b_em[e].instance < n, HK_E_INVALID, "emissive instance out of bounds");
    derive[b_em[e].instance].emitter = e;
    emitter_triangles = std::max(emitter_triangles, (b_inst[b_em[e].instance].mesh.node_count + 2u) / 3u);  // a BLAS over n triangles: 3n - 2 nodes
  }

  // the mirrors take the new level (a refusal below gives them back); with the poses on the device nothing is at motion
  std::vector<HkInstance> m_inst(b_inst, b_inst + ni);
  std::vector<HkNode> m_nodes(b_nodes, b_nodes + nin), m_enodes(b_enodes, b_enodes + nen);
  std::vector<HkEmissive> m_em(b_em, b_em + ne);
  std::vector<HkAliasEntry> m_alias(b_alias, b_alias + nal);
  std::vector<float> m_prev;
  if (!device_poses) m_prev.assign(b_prev, b_prev + 16 * (size_t)npm);
  const size_t n_materials = c->materials.size();
  auto swap_mirrors = [&] {
    c->instances.swap(m_inst); c->instance_nodes.swap(m_nodes); c->emissives.swap(m_em); c->emissive_nodes.swap(m_enodes);
    c->alias_table.swap(m_alias); c->prev_models.swap(m_prev);
  };
  auto refuse = [&](int code) {
    swap_mirrors();
    c->materials.resize(n_materials);
    return code;
  };
  swap_mirrors();
  if ((rc = take_appended_materials(c, b))) return refuse(rc);
  DynOffsets o{};
  c->dyn_blob.bytes.clear();
  c->trees_pending_on_device = n >= 2u;   // (ordering 0 of the stand-in trees alone: the device builds every ordering)
  rc = build_dynamic_region(c, c->dyn_blob, o, c->mesh.bytes);
  c->trees_pending_on_device = false;
  if (rc) return refuse(rc);
  // room: the refit's side arrays, the tree builds' scratch, the emitters' records (each waits only where it grows)
  if ((rc = reserve_refit(c, n, nal)) || (rc = reserve_tree_scratch(c, n, ne))) return refuse(rc);
  if (ne > c->df_records_cap) {
    if ((rc = sync_all(c))) return refuse(rc);
    if (c->df_records) (void)hipFree(c->df_records);
    c->df_records = nullptr;
    c->df_records_cap = 0;
    const size_t cap = (size_t)ne + ne / 4 + 16;
    if (hipMalloc((void**)&c->df_records, cap * sizeof(RefitUpdate)) != hipSuccess) {
      set_error("device allocation of %zu emitter records failed: %s", cap, hipGetErrorString(hipGetLastError()));
      return refuse(HK_E_HIP);
    }
    c->df_records_cap = cap;
  }
  uint8_t* pinned = nullptr;
  int k_stage = -1;
  if ((rc = stage(c, derive.size() * sizeof(InstanceDerive), &pinned, &k_stage))) return refuse(rc);
  memcpy(pinned, derive.data(), derive.size() * sizeof(InstanceDerive));
  // the spare slot has no room: the scene moves once, device to device behind every frame enqueued so far, to slots half again the need
  // (the layout and the 64 B per instance of a host layout's slots, scene_layout.hip finalize_scene)
  uint32_t moved_scene = 0u, launches = 0u;
  if (c->dyn_blob.bytes.size() > c->dyn_capacity) {
    const size_t need = (c->dyn_blob.bytes.size() + 64 * (size_t)n + 31) & ~(size_t)31;
    if ((rc = join_all(c)) || (rc = grow_instance_slots(c, ((need + need / 2) + 31) & ~(size_t)31))) return refuse(rc);
    moved_scene = 1u;
    ++launches;
  }

  // ---- enqueue: nothing is refused from here on.  Frames in flight keep the slot (and the allocation) they were enqueued with
  c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  const DInstance* old_instances = (const DInstance*)(c->scene_mem + (size_t)c->slot * c->dyn_capacity + c->dyn_off.instances);
  c->slot ^= 1;
  c->dyn_off = o;
  if ((rc = upload_slot_staged(c))) return rc;
  ++launches;
  point_scene_at_slot(c);   // (not repoint_scene: the refit's plane is indexed by the OLD instance set, the slot just uploaded holds the new level's previous models)
  c->instances_generation += 1;   // (the instance lists of the deformable meshes and of the pose path follow it)
  c->pd_all_ready = false;
  c->pd_boxes_host.clear();
  const RefitScene r = refit_scene(c);
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  const uint32_t orderings = c->threaded ? 8u : 1u;
  // (a tree of one leaf is what the host laid out, in every ordering: its box alone is the device's)
  launches += launch_instance_change(c->stream, r, c->rf_emissive_of_instance, device_poses ? old_instances : nullptr, (const InstanceDerive*)pinned, n, c->df_records, ne,
                                     emitter_triangles, (float4*)(base + o.tlas), n == 1u ? 1u : 0u, orderings, (float4*)(base + o.light_lo), (float4*)(base + o.light_hi),
                                     ne == 1u ? 1u : 0u);
  HK_HIP(hipGetLastError());
  {
    hk_ctx::DeformStage& st = c->df_stage[(size_t)k_stage];
    HK_HIP(hipEventRecord(st.done, c->stream));
    st.pending = true;
  }
  // the refit's side state describes the new level: which instances are at motion (the host's diff; none with the poses on the device),
  // their previous models where the layout carries the plane
  c->rf_last_moved.clear();
  if (c->prev_models.size() == 16 * (size_t)n)
    for (uint32_t i = 0; i < n; ++i)
      if (memcmp(&c->prev_models[16 * (size_t)i], c->instances[i].model, 64) != 0) c->rf_last_moved.push_back(i);
  if (!c->rf_last_moved.empty() && o.prev_models + (size_t)n * 64 <= c->dyn_capacity) {
    launch_copy_region(c->stream, c->rf_prev_models, base + o.prev_models, (size_t)n * 64);
    HK_HIP(hipGetLastError());
    ++launches;
  }
  c->rf_ready = true;
  deform_flushed(c);   // (every deformed mesh's box has just reached its instances)
  c->mirrors_stale = true;
  c->wide_tlas_dirty = true;
  c->wide_mesh_check = true;
  c->dynamic_rebuilds += 1;
  if (n >= 2u && (rc = build_trees_in_slot(c, tree_mode))) return rc;
  c->last_instance_change[0] = launches;
  c->last_instance_change[1] = n_carried;
  c->last_instance_change[2] = n - n_carried;
  c->last_instance_change[3] = moved_scene;
  return HK_OK;
}

extern "C" {
int hk_change_scene_instances(hk_ctx* c, hk_scene_builder* b, const uint32_t* origins, uint32_t n, uint32_t tree_mode) {
  return hk::change_instances_impl(c, b, origins, n, tree_mode, true);
}
// Test hook (hikari_hip_debug.h)
int hk_debug_last_instance_change(hk_ctx* c, uint32_t out[4]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 4; ++k) out[k] = c->last_instance_change[k];
  return HK_OK;
}
}  // extern "C"
