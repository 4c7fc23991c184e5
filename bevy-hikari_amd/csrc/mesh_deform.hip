// mesh_deform.hip - mesh deformation on the device (hikari_hip.h hk_update_mesh_vertices / hk_set_mesh_skin / hk_skin_mesh / hk_set_mesh_morph_targets / hk_deform_meshes / hk_deform_meshes_device; kernels in
// kernels_deform.hip, kernels_tree.hip and kernels_scene.hip; DESIGN "Mesh deformation").  The reference re-prepares a changed mesh on the CPU
// (mesh.rs:76-166: a BVH build and a re-layout of the whole mesh level); here the new vertices are written into the mesh-level region,
// the mesh tree is REFIT in every ordering that holds it (same links, every box the union of the triangle boxes below it), and the
// new mesh box goes up to the instances, emitters and both instance-level trees - all stream-ordered behind the frames enqueued before.
#include <array>
#include <string>

#include "hk_context.hpp"

using namespace hk;
using namespace hkd;

struct DeformMesh {
  HkMeshIndex mesh{};
  uint32_t n_tris = 0, max_vertices = 0, min_vertices = 0;   // vertex count accepted: [min_vertices, max_vertices]
  uint32_t n_vertices = 0;                                     // the count of the last update / of the skin (0: none yet)
  void* mem = nullptr;                                         // topology + refit planes, one allocation
  MeshTree tree{};
  float4* pos = nullptr;                                       // positions of the last update (per vertex; max_vertices)
  uint32_t* box = nullptr;                                     // the mesh box, 6 order-preserving words (kernels_deform.hip)
  std::vector<uint32_t> ids;                                   // the instances of the mesh, emitters first (host: propagate stages them)
  uint32_t n_emitters = 0;
  uint64_t ids_generation = ~0ull;
  uint64_t batch = 0;                                          // the last hk_deform_meshes call that named the mesh (hk_ctx::df_batch)
  bool deformed = false;                                       // `box` holds the current mesh box
  bool have_boxes = false;                                     // tree.tri_lo / tri_hi hold the current triangle boxes
  bool pending = false;                                        // ... and its instances have not been given it yet
  // skin (hk_set_mesh_skin)
  void* skin_mem = nullptr;
  float4 *bind_pos = nullptr, *bind_nrm = nullptr, *weights = nullptr, *joint_mats = nullptr;
  uint2* joints = nullptr;
  uint32_t skin_vertices = 0, max_joint = 0, joint_cap = 0;
  // HK_DEFORM_RECOMPUTE_NORMALS (hk_deform_meshes_device), made at the mesh's first such item: the face-vector plane (per triangle) and
  // the corner list (hk_kernels.hpp DeformItem) - the topology never changes, so neither does the list
  void* nrm_mem = nullptr;
  float4* face = nullptr;
  uint32_t *corner_off = nullptr, *corner_tri = nullptr;
  // morph targets (hk_set_mesh_morph_targets), one allocation: base planes and delta planes (3 floats per vertex, the deltas target-major
  // as the caller gave them; morph_dn NULL: none), the weights of the last morph item and the list of its active targets with the
  // list's length behind it (kernels_deform.hip k_deform_begin writes both)
  void* morph_mem = nullptr;
  float *morph_base_p = nullptr, *morph_base_n = nullptr, *morph_dp = nullptr, *morph_dn = nullptr, *morph_w = nullptr;
  uint32_t* morph_active = nullptr;
  uint32_t morph_vertices = 0, morph_targets = 0;
  // motion vectors (hk_set_mesh_motion_vectors; DESIGN 4 "Motion vectors for deforming meshes"): a second position plane.  `pos` is the
  // one the deformations write, `pos_prev` the other; the mesh's first deformation after a frame swaps them (motion_swap), so that
  // pos_prev then holds what the mesh had when that frame's primary rays were enqueued.  pos_home: the plane inside `mem`.
  void* motion_mem = nullptr;
  float4 *pos_prev = nullptr, *pos_home = nullptr;
  bool motion = false;          // opted in
  bool motion_dirty = false;    // deformed (and swapped) since the last frame's primary rays
  bool motion_live = false;     // pos_prev holds the previous positions of the frame most recently begun
};

namespace {
// every device allocation of a deformable mesh: what free_deform frees and a removed mesh hands to its caller to retire
std::array<void*, 6> allocations(const DeformMesh* d) { return {d->mem, d->skin_mem, (void*)d->joint_mats, d->nrm_mem, d->morph_mem, d->motion_mem}; }
// the deformable mesh of a record (NULL: none made yet - find_mesh makes them, one per record)
DeformMesh* lookup(const hk_ctx* c, const HkMeshIndex& m) {
  for (DeformMesh* d : c->deform)
    if (memcmp(&d->mesh, &m, sizeof(HkMeshIndex)) == 0) return d;
  return nullptr;
}
// a device array that has to grow (rarely): what is enqueued may still read the old one, so wait for it, free, allocate `want`
// elements of `elem` bytes
template <typename T, typename N>
int regrow(hk_ctx* c, T*& p, N& cap, size_t want, size_t elem) {
  int rc;
  if ((rc = sync_all(c))) return rc;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  HK_HIP(hipMalloc((void**)&p, want * elem));
  cap = (N)want;
  return HK_OK;
}
// consecutive planes of one allocation, each starting on a 256-byte boundary
inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Carve {
  uint8_t* p;
  template <typename T>
  T* take(size_t bytes) { T* q = (T*)p; p += al256(bytes); return q; }
};
}  // namespace

namespace hk {
void free_deform(hk_ctx* c) {
  for (DeformMesh* d : c->deform) {
    for (void* q : allocations(d))
      if (q) (void)hipFree(q);
    delete d;
  }
  c->deform.clear();
  for (void* q : {(void*)c->mv_table, (void*)c->mv_counter})
    if (q) (void)hipFree(q);
  c->mv_table = nullptr;
  c->mv_counter = nullptr;
  c->mv_table_cap = 0;
  c->mv_enabled = c->mv_live = 0;   // (a fresh scene drops all motion state)
  for (hk_ctx::DeformStage& s : c->df_stage) {
    if (s.p) (void)hipHostFree(s.p);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  c->df_stage.clear();
  if (c->df_records) (void)hipFree(c->df_records);
  c->df_records = nullptr;
  c->df_records_cap = 0;
  c->deform_pending = false;
  for (hipEvent_t* e : {&c->df_src_ready, &c->df_src_read}) {
    if (*e) (void)hipEventDestroy(*e);
    *e = nullptr;
  }
}
// hk_remove_meshes (scene_remove.hip): what the deformable meshes name, and their records once only `runs` are left.  A mesh whose nodes
// lie in no run left with them: its allocations are the caller's to retire (frames in flight may still refit or skin it).  The tree
// topology, refit planes, skin and morph set of a survivor are its own allocations with links local to the mesh: nothing in them moves.
void deform_mesh_records(const hk_ctx* c, std::vector<HkMeshIndex>& out) {
  for (const DeformMesh* d : c->deform) out.push_back(d->mesh);
}
// hk_change_scene_instances (scene_instances.hip): the box words of a mesh deformed on the device (NULL: the builder's box is current),
// and - that call having carried every deformed mesh's box to the new instance level - nothing left to flush
const uint32_t* deformed_mesh_box(const hk_ctx* c, const HkMeshIndex& m) {
  const DeformMesh* d = lookup(c, m);
  return d && d->deformed ? d->box : nullptr;
}
void deform_flushed(hk_ctx* c) {
  for (DeformMesh* d : c->deform) d->pending = false;
  c->deform_pending = false;
}
void rebase_deform_meshes(hk_ctx* c, const std::vector<CompactRun> runs[3], std::vector<void*>& freed) {
  size_t kept = 0;
  for (DeformMesh* d : c->deform) {
    bool survives = false;
    for (const CompactRun& r : runs[0]) survives = survives || (d->mesh.node_offset >= r.src && d->mesh.node_offset - r.src < r.count);
    if (!survives) {
      for (void* q : allocations(d))
        if (q) freed.push_back(q);
      if (d->motion) {  // (the survivors keep their planes and their state; the table is written again at the next frame with a live mesh)
        c->mv_enabled -= 1;
        c->mv_live -= d->motion_live ? 1u : 0u;
        c->scene_epoch += 1;
      }
      delete d;
      continue;
    }
    d->mesh.node_offset = compact_rebase(runs[0].data(), (uint32_t)runs[0].size(), d->mesh.node_offset);
    d->mesh.primitive = compact_rebase(runs[1].data(), (uint32_t)runs[1].size(), d->mesh.primitive);
    d->mesh.vertex = compact_rebase(runs[2].data(), (uint32_t)runs[2].size(), d->mesh.vertex);
    c->deform[kept++] = d;
  }
  c->deform.resize(kept);
}
}  // namespace hk

namespace {
// The binary tree behind a mesh tree in the `bvh` 0.7.1 flatten_custom layout (ordering 0, links local to the range): a subtree over
// [b, e) is one leaf (e = b + 1) or [navigator a][subtree of a][navigator b][subtree of b] with b = exit(a), e = exit(b).
bool mesh_topology(const HkNode* nodes, uint32_t count, uint32_t n_tris, std::vector<uint32_t>& parent, std::vector<uint32_t>& left, std::vector<uint32_t>& right,
                   std::vector<uint32_t>& first, std::vector<uint32_t>& last, std::vector<uint32_t>& leaf_parent, std::vector<uint32_t>& leaf_shape) {
  if (count != 3 * n_tris - 2) return false;
  const uint32_t ni = n_tris - 1;
  parent.assign(ni, HK_U32_MAX); left.assign(ni, 0); right.assign(ni, 0); first.assign(ni, 0); last.assign(ni, 0);
  leaf_parent.assign(n_tris, HK_U32_MAX); leaf_shape.assign(n_tris, 0);
  std::vector<uint8_t> shape_seen(n_tris, 0);
  uint32_t next_internal = 0, next_leaf = 0;
  struct Frame { uint32_t b, e, id, stage, second; };
  std::vector<Frame> stack;
  // returns the tree node of [b, e): pushes a frame for an internal node, resolves a leaf at once
  auto open = [&](uint32_t b, uint32_t e, uint32_t par, bool& ok) -> uint32_t {
    if (e - b == 1) {
      if (nodes[b].entry_index < HK_BVH_LEAF_FLAG || nodes[b].exit_index != e || next_leaf >= n_tris) { ok = false; return 0; }
      const uint32_t shape = nodes[b].entry_index - HK_BVH_LEAF_FLAG;
      if (shape >= n_tris || shape_seen[shape]) { ok = false; return 0; }
      shape_seen[shape] = 1;
      leaf_shape[next_leaf] = shape;
      leaf_parent[next_leaf] = par;
      return ni + next_leaf++;
    }
    const uint32_t a = b, bb = nodes[a].exit_index;
    if (next_internal >= ni || nodes[a].entry_index != a + 1 || !(bb > a + 1 && bb < e) || nodes[bb].entry_index != bb + 1 || nodes[bb].exit_index != e) { ok = false; return 0; }
    const uint32_t id = next_internal++;
    parent[id] = par;
    first[id] = next_leaf;
    stack.push_back({b, e, id, 0, bb});
    return id;
  };
  bool ok = true;
  if (n_tris == 1) {
    (void)open(0, 1, HK_U32_MAX, ok);
    return ok && next_leaf == 1;
  }
  (void)open(0, count, HK_U32_MAX, ok);
  while (ok && !stack.empty()) {
    Frame& f = stack.back();
    if (f.stage == 0) {
      f.stage = 1;
      const uint32_t id = f.id, b = f.b, bb = f.second;
      left[id] = open(b + 1, bb, id, ok);
    } else if (f.stage == 1) {
      f.stage = 2;
      const uint32_t id = f.id, bb = f.second, e = f.e;
      right[id] = open(bb + 1, e, id, ok);
    } else {
      last[f.id] = next_leaf - 1;
      stack.pop_back();
    }
  }
  return ok && next_internal == ni && next_leaf == n_tris;
}

// the deformable mesh named by `m` (created on first use); validates the record against the uploaded instances and the tree
int find_mesh(hk_ctx* c, const HkMeshIndex* m, DeformMesh** out) {
  bool known = false;
  uint32_t next_vertex = (uint32_t)c->vertices.size();
  for (const HkInstance& in : c->instances) {
    if (memcmp(&in.mesh, m, sizeof(HkMeshIndex)) == 0) known = true;
    if (in.mesh.vertex > m->vertex) next_vertex = std::min(next_vertex, in.mesh.vertex);
  }
  HK_REQUIRE(known, HK_E_INVALID, "no uploaded instance carries the mesh record (%u, %u, %u, %u)", m->vertex, m->primitive, m->node_offset, m->node_count);
  if ((*out = lookup(c, *m))) return HK_OK;
  HK_REQUIRE(m->node_count >= 1 && (m->node_count + 2) % 3 == 0, HK_E_UNSUPPORTED, "the mesh tree is not a binary tree in the flatten_custom layout (%u nodes)", m->node_count);
  const uint32_t n_tris = (m->node_count + 2) / 3;
  HK_REQUIRE((size_t)m->primitive + n_tris <= c->primitives.size() && (size_t)m->node_offset + m->node_count <= c->asset_nodes.size() && m->vertex < c->vertices.size(),
             HK_E_INVALID, "the mesh record lies outside the uploaded mesh arrays");
  uint32_t max_ref = 0;
  for (uint32_t t = 0; t < n_tris; ++t)
    for (int k = 0; k < 3; ++k) max_ref = std::max(max_ref, c->primitives[m->primitive + t].vertices[k].index);
  HK_REQUIRE((size_t)m->vertex + max_ref < next_vertex, HK_E_INVALID, "the mesh's triangles name vertices beyond the mesh");
  std::vector<uint32_t> parent, left, right, first, last, leaf_parent, leaf_shape;
  HK_REQUIRE(mesh_topology(c->asset_nodes.data() + m->node_offset, m->node_count, n_tris, parent, left, right, first, last, leaf_parent, leaf_shape), HK_E_UNSUPPORTED,
             "the mesh tree is not a binary tree in the flatten_custom layout");
  DeformMesh* d = new (std::nothrow) DeformMesh();
  HK_REQUIRE(d, HK_E_NOMEM, "allocation failed");
  d->mesh = *m;
  d->n_tris = n_tris;
  d->min_vertices = d->max_vertices = max_ref + 1;  // the vertices the mesh's triangles span: nothing beyond them is ever written
  const size_t n = n_tris, ni = std::max<size_t>(n - 1, 1), nv = d->max_vertices;
  (void)next_vertex;
  const auto al = al256;
  const size_t bytes = al(5 * ni * 4) + al(2 * n * 4) + al(ni * 4) + al(ni) + 2 * al((2 * n - 1) * 16) + 2 * al(n * 16) + al(nv * 16) + al(32);
  if (hipMalloc(&d->mem, bytes) != hipSuccess) {
    delete d;
    HK_REQUIRE(false, HK_E_NOMEM, "device allocation of %zu bytes failed", bytes);
  }
  Carve cv{(uint8_t*)d->mem};
  uint32_t* topo = cv.take<uint32_t>(5 * ni * 4);
  d->tree.n = n_tris;
  d->tree.parent = topo; d->tree.left = topo + ni; d->tree.right = topo + 2 * ni; d->tree.first = topo + 3 * ni; d->tree.last = topo + 4 * ni;
  uint32_t* leaves = cv.take<uint32_t>(2 * n * 4);
  d->tree.leaf_parent = leaves; d->tree.leaf_shape = leaves + n;
  d->tree.arrived = cv.take<uint32_t>(ni * 4);
  d->tree.swap = cv.take<uint8_t>(ni);
  d->tree.node_lo = cv.take<float4>((2 * n - 1) * 16);
  d->tree.node_hi = cv.take<float4>((2 * n - 1) * 16);
  d->tree.tri_lo = cv.take<float4>(n * 16);
  d->tree.tri_hi = cv.take<float4>(n * 16);
  d->pos = d->pos_home = cv.take<float4>(nv * 16);
  d->box = cv.take<uint32_t>(32);
  c->deform.push_back(d);  // (owned by the context from here on, freed by free_deform)
  std::vector<uint32_t> host(5 * ni + 2 * n, 0);
  auto put = [&](const std::vector<uint32_t>& v, size_t at) { std::copy(v.begin(), v.end(), host.begin() + at); };
  put(parent, 0); put(left, ni); put(right, 2 * ni); put(first, 3 * ni); put(last, 4 * ni);
  HK_HIP(hipMemcpy(topo, host.data(), 5 * ni * 4, hipMemcpyHostToDevice));
  std::copy(leaf_parent.begin(), leaf_parent.end(), host.begin());
  std::copy(leaf_shape.begin(), leaf_shape.end(), host.begin() + n);
  HK_HIP(hipMemcpy(leaves, host.data(), 2 * n * 4, hipMemcpyHostToDevice));
  *out = d;
  return HK_OK;
}

// the instances of the mesh (emitters first) as the uploaded scene has them; redone after every hk_upload_instances
int mesh_instances(hk_ctx* c, DeformMesh* d) {
  if (d->ids_generation == c->instances_generation) return HK_OK;
  std::vector<uint8_t> is_emitter(c->instances.size(), 0);
  for (const HkEmissive& e : c->emissives)
    if (e.instance < c->instances.size()) is_emitter[e.instance] = 1;
  std::vector<uint32_t> ids;
  for (int pass = 0; pass < 2; ++pass)
    for (uint32_t i = 0; i < c->instances.size(); ++i)
      if (memcmp(&c->instances[i].mesh, &d->mesh, sizeof(HkMeshIndex)) == 0 && is_emitter[i] == (pass == 0 ? 1 : 0)) ids.push_back(i);
  uint32_t n_emitters = 0;
  for (uint32_t i : ids) n_emitters += is_emitter[i];
  d->ids.swap(ids);
  d->n_emitters = n_emitters;
  d->ids_generation = c->instances_generation;
  return HK_OK;
}

}  // namespace
// a pinned staging buffer of at least `bytes`: one whose last reader has passed (hipEventQuery: no host wait), or a new one
int hk::stage(hk_ctx* c, size_t bytes, uint8_t** out, int* k_out) {
  int k = -1;
  for (size_t i = 0; i < c->df_stage.size() && k < 0; ++i) {
    hk_ctx::DeformStage& s = c->df_stage[i];
    if (s.pending && hipEventQuery(s.done) != hipSuccess) continue;
    s.pending = false;
    if (s.cap >= bytes) k = (int)i;
  }
  if (k < 0) {
    for (size_t i = 0; i < c->df_stage.size() && k < 0; ++i)
      if (!c->df_stage[i].pending) k = (int)i;  // (free but too small: grown below)
    if (k < 0) {
      c->df_stage.emplace_back();
      k = (int)c->df_stage.size() - 1;
    }
    hk_ctx::DeformStage& s = c->df_stage[(size_t)k];
    if (s.p) (void)hipHostFree(s.p);
    s.p = nullptr;
    s.cap = 0;
    const size_t cap = bytes + bytes / 4 + 256;
    HK_HIP(hipHostMalloc((void**)&s.p, cap, hipHostMallocDefault));
    s.cap = cap;
  }
  hk_ctx::DeformStage& s = c->df_stage[(size_t)k];
  if (!s.done) HK_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  *out = s.p;
  *k_out = k;
  return HK_OK;
}

// a source of hk_deform_meshes_device / hk_update_textures_device: aligned, memory the context's device can read - its own, or host memory
// mapped for it - and `extent` bytes from `p` on inside the allocation, so that no launch can fault on what a caller named by mistake
int hk::check_source(hk_ctx* c, uint32_t item, const char* what, const void* p, size_t align, size_t extent) {
  HK_REQUIRE(((uintptr_t)p & (align - 1)) == 0, HK_E_INVALID, "item %u: the %s at %p are not aligned to %zu bytes", item, what, p, align);
  hipPointerAttribute_t a{};
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) (void)hipGetLastError();  // (plain host memory: an error on some runtimes, hipMemoryTypeUnregistered on others)
  HK_REQUIRE(e == hipSuccess && ((a.type == hipMemoryTypeDevice && a.device == c->device) || a.type == hipMemoryTypeHost), HK_E_INVALID,
             "item %u: the %s at %p are neither memory of device %d nor host memory the device can access", item, what, p, c->device);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return HK_OK;
  }
  HK_REQUIRE((const uint8_t*)p + extent <= (const uint8_t*)base + size, HK_E_INVALID, "item %u: the %s reach %zu bytes beyond their allocation", item, what,
             (size_t)(((const uint8_t*)p + extent) - ((const uint8_t*)base + size)));
  return HK_OK;
}

namespace {
inline uint32_t stride_of(uint32_t bytes) { return bytes ? bytes : 12u; }

// the corner list and the face plane of a mesh's recomputed normals, from the primitive mirror (indices never change): per vertex the
// triangles that name it, ascending, one entry per corner - the order k_deform_normals sums in
int corner_list(hk_ctx* c, DeformMesh* d) {
  const size_t nv = d->max_vertices, nt = d->n_tris;
  std::vector<uint32_t> host(nv + 1 + 3 * nt, 0);
  uint32_t* off = host.data();
  uint32_t* tri = host.data() + nv + 1;
  const HkPrimitive* prims = c->primitives.data() + d->mesh.primitive;
  for (size_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k) off[prims[t].vertices[k].index + 1] += 1;
  for (size_t v = 0; v < nv; ++v) off[v + 1] += off[v];
  std::vector<uint32_t> at(off, off + nv);
  for (size_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k) tri[at[prims[t].vertices[k].index]++] = (uint32_t)t;
  const size_t bytes = al256(nt * 16) + host.size() * 4;
  HK_REQUIRE(hipMalloc(&d->nrm_mem, bytes) == hipSuccess, HK_E_NOMEM, "device allocation of %zu bytes failed", bytes);
  Carve cv{(uint8_t*)d->nrm_mem};
  d->face = cv.take<float4>(nt * 16);
  d->corner_off = cv.take<uint32_t>(host.size() * 4);
  d->corner_tri = d->corner_off + nv + 1;
  if (hipMemcpy(d->corner_off, host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d->nrm_mem);
    d->nrm_mem = nullptr;
    HK_REQUIRE(false, HK_E_HIP, "copying the corner list failed: %s", hipGetErrorString(hipGetLastError()));
  }
  return HK_OK;
}

// common front of the three calls: the scene as laid out, the refit's side arrays, the mesh
int begin(hk_ctx* c, const HkMeshIndex* m, DeformMesh** d) {
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = find_mesh(c, m, d))) return rc;
  return mesh_instances(c, *d);
}

// what every deformation leaves behind on the host side, whatever it wrote: the mirrors are stale, the wide records of the mesh trees
// `keys` (sorted (node_offset, node_count)) are derived again (context.hip ensure_wide), the instance tree's too
void mark_deformed(hk_ctx* c, const std::vector<std::pair<uint32_t, uint32_t>>& keys) {
  c->meshes_deformed = true;
  c->mirrors_stale = true;
  update_shared_transform(c);  // (the one-level tree is not walked from here on)
  c->wide_meshes.erase(std::remove_if(c->wide_meshes.begin(), c->wide_meshes.end(),
                                      [&](const std::pair<uint32_t, uint32_t>& m) { return std::binary_search(keys.begin(), keys.end(), m); }),
                       c->wide_meshes.end());
  c->wide_mesh_check = true;
  c->wide_tlas_dirty = true;
}

// motion vectors: the mesh's first deformation since the last frame's primary rays writes the OTHER plane - what `pos` held becomes the
// previous positions of the next frame; later deformations before that frame overwrite the current plane.  No copy, no launch.
// Called behind join_all, right in front of the launch that writes d->pos.
void motion_swap(DeformMesh* d) {
  if (!d->motion || d->motion_dirty) return;
  std::swap(d->pos, d->pos_prev);
  d->motion_dirty = true;
}

// the device work after the vertices of `d` are in `d->pos` (and its normals in the normal plane): triangles, the mesh tree in every
// ordering.  The instance level follows once for all meshes deformed before the next frame (flush_deform).
int refit_mesh(hk_ctx* c, DeformMesh* d) {
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  uint8_t* sbase = c->scene_mem + slots;
  const uint32_t p0 = d->mesh.primitive;
  launch_mesh_triangles(c->stream, d->pos, (float4*)(sbase + c->mesh.v0) + p0, (float4*)(sbase + c->mesh.v1) + p0, (float4*)(sbase + c->mesh.v2) + p0, d->n_tris, d->tree.tri_lo,
                        d->tree.tri_hi);
  launch_mesh_tree_refit(c->stream, d->tree, (float4*)(sbase + c->mesh.nodes) + 2 * (size_t)d->mesh.node_offset, 2 * c->mesh.node_cap, c->threaded ? 8u : 1u);
  HK_HIP(hipGetLastError());
  d->deformed = d->pending = d->have_boxes = true;
  c->deform_pending = true;
  return HK_OK;
}

// one deformation: `fill` enqueues the vertex kernel (positions into d->pos, normals into the normal plane, the mesh box into d->box)
template <typename Fill>
int deform(hk_ctx* c, DeformMesh* d, int k, Fill fill) {
  int rc;
  // the mesh-level region has ONE copy: the writes go behind every frame enqueued so far on every stream that reads the scene (the
  // side stream's direct-light dispatches, the post stream; the pipelined primary rays are behind the main stream already) - stream
  // waits, not host waits
  if ((rc = join_all(c))) return rc;
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  float4* vn = (float4*)(c->scene_mem + slots + c->mesh.vn) + d->mesh.vertex;
  HK_HIP(hipMemsetAsync(d->box, 0xFF, 12, c->stream));
  HK_HIP(hipMemsetAsync(d->box + 3, 0, 12, c->stream));
  fill(vn);
  HK_HIP(hipGetLastError());
  if ((rc = refit_mesh(c, d))) return rc;
  hk_ctx::DeformStage& st = c->df_stage[(size_t)k];
  HK_HIP(hipEventRecord(st.done, c->stream));
  st.pending = true;
  mark_deformed(c, {std::make_pair(d->mesh.node_offset, d->mesh.node_count)});
  return HK_OK;
}

// Many meshes in one call (hikari_hip.h): what the single calls do for each item, as five launches over all of them
// (kernels_deform.hip launch_deform_batch).  Everything the device reads of the call - the item table, the workgroup tables of the
// three launch shapes, every item's positions / normals / joint matrices / morph weights - travels in ONE pinned staging block.
// hk_deform_meshes_device is the same batch with `device` set: the items' data stays where the caller has it (validated first: memory the
// device can read, aligned, strided), only the tables are staged, `producer` (or NULL) is ordered against the context's stream by two
// events, and flagged items recompute their normals in a sixth launch.
// Three steps: plan_batch validates and sizes, stage_batch fills the staging block, enqueue_batch launches.  The WHOLE batch is validated
// before anything is enqueued or written: nothing but plan_batch refuses an item.
inline bool is_skin(uint32_t kind) { return kind == HK_DEFORM_SKIN || kind == HK_DEFORM_MORPH_SKIN; }
inline bool is_morph(uint32_t kind) { return kind == HK_DEFORM_MORPH || kind == HK_DEFORM_MORPH_SKIN; }
inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }
struct DeformPlan {
  std::vector<DeformMesh*> meshes;   // per item
  uint32_t orderings = 1, total_vertices = 0, total_tris = 0;
  size_t data_bytes = 0;             // the items' data in the staging block (host sources only)
  size_t blocks[4] = {0, 0, 0, 0};   // vertex, triangle, node workgroups; the vertex workgroups of the items that recompute normals
  // the staging block (stage_batch): item table | vertex, triangle, node and normal workgroups | the items' data
  int stage = 0;
  DeformItem* table = nullptr;
  SegmentBlock* bl[4] = {nullptr, nullptr, nullptr, nullptr};
};

int plan_batch(hk_ctx* c, const HkMeshDeformDevice* items, uint32_t n, bool device, DeformPlan& p) {
  int rc;
  c->df_batch += 1;
  p.meshes.assign(n, nullptr);
  p.orderings = c->threaded ? 8u : 1u;
  for (uint32_t i = 0; i < n; ++i) {
    const HkMeshDeformDevice& it = items[i];
    HK_REQUIRE(it.kind <= HK_DEFORM_MORPH_SKIN, HK_E_INVALID, "item %u: unknown kind %u", i, it.kind);
    const bool skins = is_skin(it.kind), morphs = is_morph(it.kind);
    HK_REQUIRE(it.data && it.count, HK_E_INVALID, "item %u: NULL data or a count of zero", i);
    HK_REQUIRE(it.kind != HK_DEFORM_SKIN || !it.normals, HK_E_INVALID, "item %u: a skin item takes no normals", i);
    HK_REQUIRE(it.kind != HK_DEFORM_MORPH || !it.normals, HK_E_INVALID, "item %u: a morph item takes no normals (its data are the weights)", i);
    HK_REQUIRE(it.kind != HK_DEFORM_MORPH_SKIN || it.normals, HK_E_INVALID, "item %u: a morph + skin item names its weights in `normals`: NULL", i);
    const bool recompute = (it.flags & HK_DEFORM_RECOMPUTE_NORMALS) != 0;
    if (device) {
      HK_REQUIRE(!(it.flags & ~HK_DEFORM_RECOMPUTE_NORMALS), HK_E_INVALID, "item %u: unknown flag bits 0x%x", i, it.flags & ~HK_DEFORM_RECOMPUTE_NORMALS);
      HK_REQUIRE(!recompute || !morphs, HK_E_INVALID, "item %u: a morph item cannot recompute its normals (HK_DEFORM_RECOMPUTE_NORMALS is for vertex items)", i);
      HK_REQUIRE(!recompute || it.kind == HK_DEFORM_VERTICES, HK_E_INVALID, "item %u: a skin item cannot recompute its normals (the skin transforms them)", i);
      HK_REQUIRE(!recompute || !it.normals, HK_E_INVALID, "item %u: normals given together with HK_DEFORM_RECOMPUTE_NORMALS", i);
      if (skins) {
        HK_REQUIRE(it.data_stride == 0 || it.data_stride == 64, HK_E_INVALID, "item %u: joint matrices are contiguous (a stride of 0 or 64 bytes, not %u)", i, it.data_stride);
        HK_REQUIRE(!morphs || it.normals_stride == 0 || it.normals_stride == 4, HK_E_INVALID, "item %u: morph weights are contiguous (a stride of 0 or 4 bytes, not %u)", i,
                   it.normals_stride);
      } else if (morphs) {
        HK_REQUIRE(it.data_stride == 0 || it.data_stride == 4, HK_E_INVALID, "item %u: morph weights are contiguous (a stride of 0 or 4 bytes, not %u)", i, it.data_stride);
      } else {
        for (const uint32_t stride : {it.data_stride, it.normals ? it.normals_stride : 0u})
          HK_REQUIRE(stride == 0 || (stride >= 12 && stride % 4 == 0), HK_E_INVALID, "item %u: a stride of %u bytes (0, or a multiple of 4 from 12 on)", i, stride);
      }
    }
    DeformMesh* d = nullptr;
    if (skins || morphs) {
      d = lookup(c, it.mesh);
      HK_REQUIRE(!morphs || (d && d->morph_vertices), HK_E_INVALID, "item %u: no morph set for this mesh (hk_set_mesh_morph_targets)", i);
      HK_REQUIRE(it.kind != HK_DEFORM_MORPH || it.count == d->morph_targets, HK_E_INVALID, "item %u: the morph set has %u targets but %u weights were given", i,
                 d->morph_targets, it.count);
      HK_REQUIRE(!skins || (d && d->skin_vertices), HK_E_INVALID, "item %u: no skin set for this mesh (hk_set_mesh_skin)", i);
      HK_REQUIRE(!(skins && morphs) || d->skin_vertices == d->morph_vertices, HK_E_INVALID, "item %u: the skin has %u vertices, the morph set %u", i, d->skin_vertices,
                 d->morph_vertices);
      HK_REQUIRE(!skins || d->max_joint < it.count, HK_E_INVALID, "item %u: the skin names joint %u but only %u joint matrices were given", i, d->max_joint, it.count);
    }
    if ((rc = find_mesh(c, &it.mesh, &d)) || (rc = mesh_instances(c, d))) {
      const std::string why = hk_last_error();
      set_error("item %u: %s", i, why.c_str());
      return rc;
    }
    HK_REQUIRE(it.kind != HK_DEFORM_VERTICES || (it.count >= d->min_vertices && it.count <= d->max_vertices), HK_E_INVALID,
               "item %u: the mesh has between %u and %u vertices, not %u", i, d->min_vertices, d->max_vertices, it.count);
    HK_REQUIRE(d->batch != c->df_batch, HK_E_INVALID, "item %u: the mesh record (%u, %u, %u, %u) is named twice in one batch", i, it.mesh.vertex, it.mesh.primitive,
               it.mesh.node_offset, it.mesh.node_count);
    d->batch = c->df_batch;
    p.meshes[i] = d;
    const uint32_t nv = morphs ? d->morph_vertices : skins ? d->skin_vertices : it.count;
    if (device) {  // (the counts are known to be the mesh's: the extents below are what the kernels will read)
      if (skins) {
        if ((rc = check_source(c, i, "joint matrices", it.data, 16, (size_t)it.count * 64))) return rc;
        if (morphs && (rc = check_source(c, i, "morph weights", it.normals, 4, (size_t)d->morph_targets * 4))) return rc;
      } else if (morphs) {
        if ((rc = check_source(c, i, "morph weights", it.data, 4, (size_t)d->morph_targets * 4))) return rc;
      } else {
        if ((rc = check_source(c, i, "positions", it.data, 4, (size_t)(nv - 1) * stride_of(it.data_stride) + 12))) return rc;
        if (it.normals && (rc = check_source(c, i, "normals", it.normals, 4, (size_t)(nv - 1) * stride_of(it.normals_stride) + 12))) return rc;
      }
      if (recompute) p.blocks[3] += (nv + 255u) / 256u;
    } else {  // (host sources travel in the staging block: morph weights, then the palette or the vertex planes)
      if (morphs) p.data_bytes += al16((size_t)d->morph_targets * 4);
      if (skins) p.data_bytes += (size_t)it.count * 64;
      else if (!morphs) p.data_bytes += al16((size_t)it.count * 12) * (it.normals ? 2 : 1);
    }
    p.total_vertices += nv;
    p.total_tris += d->n_tris;
    p.blocks[0] += (nv + 255u) / 256u;
    p.blocks[1] += (d->n_tris + 255u) / 256u;
    p.blocks[2] += ((size_t)(2u * d->n_tris - 1u) * p.orderings + 255u) / 256u;
  }
  return HK_OK;
}

int stage_batch(hk_ctx* c, const HkMeshDeformDevice* items, uint32_t n, bool device, bool producer, DeformPlan& p) {
  int rc;
  // what has to grow first (a mesh's first recomputed normals, the first skinning of a mesh, a longer palette): behind a wait
  for (uint32_t i = 0; i < n; ++i) {
    DeformMesh* d = p.meshes[i];
    if ((items[i].flags & HK_DEFORM_RECOMPUTE_NORMALS) && !d->nrm_mem && ((rc = sync_all(c)) || (rc = corner_list(c, d)))) return rc;
    if (is_skin(items[i].kind) && items[i].count > d->joint_cap && (rc = regrow(c, d->joint_mats, d->joint_cap, items[i].count, 64))) return rc;
  }
  if (producer)
    for (hipEvent_t* e : {&c->df_src_ready, &c->df_src_read})
      if (!*e) HK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  const size_t table_bytes = al256(n * sizeof(DeformItem));
  const size_t block_bytes = al256((p.blocks[0] + p.blocks[1] + p.blocks[2] + p.blocks[3]) * sizeof(SegmentBlock));
  uint8_t* st = nullptr;
  if ((rc = stage(c, table_bytes + block_bytes + p.data_bytes, &st, &p.stage))) return rc;
  p.table = (DeformItem*)st;
  p.bl[0] = (SegmentBlock*)(st + table_bytes);
  for (int s = 1; s < 4; ++s) p.bl[s] = p.bl[s - 1] + p.blocks[s - 1];
  uint8_t* data = st + table_bytes + block_bytes;
  auto staged = [&](const void* src, size_t bytes, size_t advance) {  // a host source into the block; a device source stays where it is
    if (device) return src;
    memcpy(data, src, bytes);
    data += advance;
    return (const void*)(data - advance);
  };
  uint8_t* sbase = c->scene_mem + (c->two_slots ? 2 : 1) * c->dyn_capacity;
  size_t at[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const HkMeshDeformDevice& it = items[i];
    DeformMesh* d = p.meshes[i];
    DeformItem t{};
    t.pos_stride = t.nrm_stride = 3u;
    t.kind = it.kind;
    t.n_tris = d->n_tris;
    const bool skins = is_skin(it.kind), morphs = is_morph(it.kind);
    if (morphs) {  // (the weights: `data` of a morph item, `normals` of a morph + skin item)
      const size_t bytes = (size_t)d->morph_targets * 4;
      t.n_vertices = d->morph_vertices;
      t.n_targets = d->morph_targets;
      t.morph_src = (const float*)staged(skins ? it.normals : it.data, bytes, al16(bytes));
      t.morph_base_p = d->morph_base_p; t.morph_base_n = d->morph_base_n; t.morph_dp = d->morph_dp; t.morph_dn = d->morph_dn;
      t.morph_w = d->morph_w; t.morph_active = d->morph_active;
    }
    if (skins) {
      t.n_vertices = d->skin_vertices;
      t.n_joints = it.count;
      t.palette = (const float4*)staged(it.data, (size_t)it.count * 64, (size_t)it.count * 64);
      t.joint_mats = d->joint_mats;
      t.bind_pos = d->bind_pos; t.bind_nrm = d->bind_nrm; t.weights = d->weights; t.joints = d->joints;
    } else if (!morphs) {
      const size_t plane = (size_t)it.count * 12;  // (of a host source: packed)
      t.n_vertices = it.count;
      t.positions = (const float*)staged(it.data, plane, al16(plane));
      if (it.normals) t.normals = (const float*)staged(it.normals, plane, al16(plane));
      t.pos_stride = stride_of(it.data_stride) / 4u;
      t.nrm_stride = stride_of(it.normals_stride) / 4u;
      if (it.flags & HK_DEFORM_RECOMPUTE_NORMALS) {
        t.face = d->face;
        t.corner_off = d->corner_off;
        t.corner_tri = d->corner_tri;
        for (uint32_t first = 0; first < t.n_vertices; first += 256) p.bl[3][at[3]++] = SegmentBlock{i, first};
      }
    }
    t.vn = (float4*)(sbase + c->mesh.vn) + d->mesh.vertex;   // (t.pos: enqueue_batch, behind the motion swap)
    t.box = d->box;
    t.v0 = (float4*)(sbase + c->mesh.v0) + d->mesh.primitive;
    t.v1 = (float4*)(sbase + c->mesh.v1) + d->mesh.primitive;
    t.v2 = (float4*)(sbase + c->mesh.v2) + d->mesh.primitive;
    t.tree = d->tree;
    t.nodes = (float4*)(sbase + c->mesh.nodes) + 2 * (size_t)d->mesh.node_offset;
    p.table[i] = t;
    const size_t threads[3] = {t.n_vertices, t.n_tris, (size_t)(2u * t.n_tris - 1u) * p.orderings};
    for (int s = 0; s < 3; ++s)
      for (size_t first = 0; first < threads[s]; first += 256) p.bl[s][at[s]++] = SegmentBlock{i, (uint32_t)first};
  }
  return HK_OK;
}

int enqueue_batch(hk_ctx* c, uint32_t n, hipStream_t producer, const DeformPlan& p) {
  int rc;
  if ((rc = join_all(c))) return rc;  // behind every frame enqueued so far on every stream that reads the scene (stream waits), as a single deformation is
  if (producer) {  // what the producer has enqueued on the sources so far comes first; it may write them again once the vertex launch has read them
    HK_HIP(hipEventRecord(c->df_src_ready, producer));
    HK_HIP(hipStreamWaitEvent(c->stream, c->df_src_ready, 0));
  }
  c->scene_epoch += n;  // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining - a refusal above leaves it alone)
  for (uint32_t i = 0; i < n; ++i) {  // (motion vectors: the plane this batch writes - the staged table is the host's until the launch)
    motion_swap(p.meshes[i]);
    p.table[i].pos = p.meshes[i]->pos;
  }
  launch_deform_batch(c->stream, p.table, n, p.bl[0], (uint32_t)p.blocks[0], p.bl[1], (uint32_t)p.blocks[1], p.bl[2], (uint32_t)p.blocks[2], 2 * c->mesh.node_cap, p.orderings,
                      producer ? c->df_src_read : nullptr, p.bl[3], (uint32_t)p.blocks[3]);
  HK_HIP(hipGetLastError());
  if (producer) HK_HIP(hipStreamWaitEvent(producer, c->df_src_read, 0));
  hk_ctx::DeformStage& stg = c->df_stage[(size_t)p.stage];
  HK_HIP(hipEventRecord(stg.done, c->stream));
  stg.pending = true;
  std::vector<std::pair<uint32_t, uint32_t>> keys(n);
  for (uint32_t i = 0; i < n; ++i) {
    DeformMesh* d = p.meshes[i];
    d->n_vertices = p.table[i].n_vertices;
    d->deformed = d->pending = d->have_boxes = true;
    keys[i] = std::make_pair(d->mesh.node_offset, d->mesh.node_count);
  }
  c->deform_pending = true;
  std::sort(keys.begin(), keys.end());
  mark_deformed(c, keys);
  c->last_deform[0] = n;
  c->last_deform[1] = p.total_vertices;
  c->last_deform[2] = p.total_tris;
  c->last_deform[3] = p.blocks[3] ? 6u : 5u;  // begin, vertices, triangles, (normals,) boxes, emit
  return HK_OK;
}

int deform_batch(hk_ctx* c, const HkMeshDeformDevice* items, uint32_t n, bool device, hipStream_t producer) {
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  DeformPlan p;
  if ((rc = plan_batch(c, items, n, device, p))) return rc;
  if ((rc = stage_batch(c, items, n, device, producer != nullptr, p))) return rc;
  return enqueue_batch(c, n, producer, p);
}

// the new boxes of the meshes selected by `which` to their instances and emitters - ONE launch each over the instances / the emitters of
// all those meshes, however many - then ONE refit of the instance tree and the light tree
template <typename Which>
int propagate(hk_ctx* c, Which which) {
  const hkd::RefitScene r = refit_scene(c);
  uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  size_t n_entries = 0, n_emitters = 0;
  uint32_t emitter_triangles = 0;
  int rc;
  for (DeformMesh* d : c->deform) {
    if (!which(d)) continue;
    if ((rc = mesh_instances(c, d))) return rc;
    n_entries += d->ids.size();
    n_emitters += d->n_emitters;
    if (d->n_emitters) emitter_triangles = std::max(emitter_triangles, d->n_tris);
  }
  MeshInstanceEntry* entries = nullptr;
  int k = -1;
  if (n_entries) {
    if (n_emitters > c->df_records_cap && (rc = regrow(c, c->df_records, c->df_records_cap, n_emitters + n_emitters / 4 + 16, sizeof(RefitUpdate)))) return rc;
    uint8_t* st = nullptr;
    if ((rc = stage(c, n_entries * sizeof(MeshInstanceEntry), &st, &k))) return rc;
    entries = (MeshInstanceEntry*)st;
    size_t at = 0;
    uint32_t record = 0;
    for (DeformMesh* d : c->deform) {
      if (!which(d)) continue;
      for (size_t i = 0; i < d->ids.size(); ++i) entries[at++] = MeshInstanceEntry{d->ids[i], i < d->n_emitters ? record++ : HK_U32_MAX, d->box};
    }
  }
  for (DeformMesh* d : c->deform)
    if (which(d)) d->pending = false;
  c->last_deform[4] = launch_mesh_propagate(c->stream, r, entries, (uint32_t)n_entries, c->df_records, (uint32_t)n_emitters, emitter_triangles, (float4*)(base + c->dyn_off.tlas),
                                            (uint32_t)c->instance_nodes.size(), c->threaded ? 8u : 1u, (float4*)(base + c->dyn_off.light_lo),
                                            (float4*)(base + c->dyn_off.light_hi), (uint32_t)c->emissive_nodes.size());
  HK_HIP(hipGetLastError());
  if (k >= 0) {
    hk_ctx::DeformStage& st = c->df_stage[(size_t)k];
    HK_HIP(hipEventRecord(st.done, c->stream));
    st.pending = true;
  }
  c->deform_pending = false;
  return HK_OK;
}
}  // namespace

// hk_refit_scene_instances has just refit the instance level from the builder's mesh boxes: every deformed mesh's device box again
int hk::repropagate_deformed(hk_ctx* c) { return propagate(c, [](const DeformMesh* d) { return d->deformed; }); }

// Once before whatever reads the instance level next (context.hip ready: every frame path; hk_rebuild_scene_trees; the read hooks):
// the instances, emitters and trees of every mesh deformed since the last flush, however many deformation calls came in between.
int hk::flush_deform(hk_ctx* c) {
  if (!c->deform_pending) return HK_OK;
  int rc;
  if ((rc = prepare_refit(c))) return rc;
  if ((rc = begin_device_update(c))) return rc;   // (frames in flight keep the instance-level slot they were enqueued with)
  return propagate(c, [](const DeformMesh* d) { return d->pending; });
}

// Motion vectors, in front of a frame's first primary rays (hk_context.hpp): a mesh deformed since the last frame's rays is live, every
// other one is not (a mesh not deformed between two frames has no motion in the second: its pixels take the rigid formula again).  A
// live mesh's previous plane changes with every swap, so the instance table is staged and written again - on the main stream, behind
// every earlier frame's pass - in each frame that has a live mesh; a frame without one launches and writes nothing.
int hk::motion_frame(hk_ctx* c) {
  if (c->mv_seen == c->mv_frame) return HK_OK;   // (later row pieces of the same frame)
  c->mv_seen = c->mv_frame;
  c->last_motion[0] = c->last_motion[1] = 0;
  if (!c->mv_enabled) return HK_OK;
  uint32_t live = 0;
  bool changed = false;
  for (DeformMesh* d : c->deform) {
    if (!d->motion) continue;
    changed = changed || d->motion_dirty != d->motion_live;
    d->motion_live = d->motion_dirty;
    d->motion_dirty = false;
    live += d->motion_live ? 1u : 0u;
  }
  c->mv_live = c->last_motion[1] = live;
  if (changed) c->scene_epoch += 1;
  if (!live) return HK_OK;
  int rc;
  const size_t n = c->instances.size();
  if (n > c->mv_table_cap && (rc = regrow(c, c->mv_table, c->mv_table_cap, n + n / 4 + 16, sizeof(MotionEntry)))) return rc;
  if (c->mv_count && !c->mv_counter) HK_HIP(hipMalloc((void**)&c->mv_counter, sizeof(unsigned int)));
  uint8_t* st = nullptr;
  int k = 0;
  if ((rc = stage(c, n * sizeof(MotionEntry), &st, &k))) return rc;
  MotionEntry* entries = (MotionEntry*)st;
  for (size_t i = 0; i < n; ++i) {
    const DeformMesh* d = lookup(c, c->instances[i].mesh);
    entries[i] = d && d->motion_live ? MotionEntry{d->pos_prev, d->max_vertices, 0u} : MotionEntry{nullptr, 0u, 0u};
  }
  launch_copy_region(c->stream, c->mv_table, st, n * sizeof(MotionEntry));
  HK_HIP(hipGetLastError());
  hk_ctx::DeformStage& stg = c->df_stage[(size_t)k];
  HK_HIP(hipEventRecord(stg.done, c->stream));
  stg.pending = true;
  if (c->mv_count) HK_HIP(hipMemsetAsync(c->mv_counter, 0, sizeof(unsigned int), c->stream));
  return HK_OK;
}

int hk::motion_pass(hk_ctx* c, hipStream_t st, const DFrame& fr, const GBuffer& g, float jitter_x, float jitter_y, int y0, int y1) {
  if (!c->mv_live || y1 <= y0) return HK_OK;
  MotionTable mt;
  mt.entries = c->mv_table;
  mt.n_instances = (uint32_t)std::min(c->instances.size(), c->mv_table_cap);
  mt.rewritten = c->mv_count ? c->mv_counter : nullptr;
  launch_motion_velocity(st, c->scene, fr, c->view.inverse_view_proj, c->view.view_proj, c->pview.view_proj, c->d_prev_models, jitter_x, jitter_y, g, mt, y0, y1);
  HK_HIP(hipGetLastError());
  c->last_motion[0] += 1;
  return HK_OK;
}

extern "C" {

int hk_update_mesh_vertices(hk_ctx* c, const HkMeshIndex* mesh, uint32_t n_vertices, const float* positions, const float* normals) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && mesh && positions && n_vertices, HK_E_INVALID, "NULL argument or no vertices");
  DeformMesh* d = nullptr;
  int rc;
  if ((rc = begin(c, mesh, &d))) return rc;
  HK_REQUIRE(n_vertices >= d->min_vertices && n_vertices <= d->max_vertices, HK_E_INVALID, "the mesh has between %u and %u vertices, not %u", d->min_vertices,
             d->max_vertices, n_vertices);
  uint8_t* st = nullptr;
  int k = 0;
  const size_t plane = (size_t)n_vertices * 12, nplane = (plane + 15) & ~(size_t)15;
  if ((rc = stage(c, nplane + (normals ? plane : 0), &st, &k))) return rc;
  memcpy(st, positions, plane);
  if (normals) memcpy(st + nplane, normals, plane);
  d->n_vertices = n_vertices;
  return deform(c, d, k, [&](float4* vn) {
    motion_swap(d);
    launch_mesh_stage(c->stream, (const float*)st, normals ? (const float*)(st + nplane) : nullptr, n_vertices, d->pos, vn, d->box);
  });
}

int hk_set_mesh_skin(hk_ctx* c, const HkMeshIndex* mesh, uint32_t n_vertices, const float* bind_positions, const float* bind_normals, const uint16_t* joint_indices,
                     const float* joint_weights) {
  HK_REQUIRE(c && mesh && bind_positions && bind_normals && joint_indices && joint_weights && n_vertices, HK_E_INVALID, "NULL argument or no vertices");
  DeformMesh* d = nullptr;
  int rc;
  if ((rc = begin(c, mesh, &d))) return rc;
  HK_REQUIRE(n_vertices >= d->min_vertices && n_vertices <= d->max_vertices, HK_E_INVALID, "the mesh has between %u and %u vertices, not %u", d->min_vertices,
             d->max_vertices, n_vertices);
  const size_t n = n_vertices;
  std::vector<float4> bp(n), bn(n), w(n);
  std::vector<uint2> j(n);
  uint32_t max_joint = 0;
  for (size_t v = 0; v < n; ++v) {
    bp[v] = make_float4(bind_positions[3 * v], bind_positions[3 * v + 1], bind_positions[3 * v + 2], 0.0f);
    bn[v] = make_float4(bind_normals[3 * v], bind_normals[3 * v + 1], bind_normals[3 * v + 2], 0.0f);
    w[v] = make_float4(joint_weights[4 * v], joint_weights[4 * v + 1], joint_weights[4 * v + 2], joint_weights[4 * v + 3]);
    const uint16_t* q = joint_indices + 4 * v;
    j[v] = make_uint2((uint32_t)q[0] | ((uint32_t)q[1] << 16), (uint32_t)q[2] | ((uint32_t)q[3] << 16));
    for (int t = 0; t < 4; ++t) max_joint = std::max<uint32_t>(max_joint, q[t]);
  }
  if ((rc = sync_all(c))) return rc;  // (a skin set again: the kernels enqueued so far may still read the old one)
  if (d->skin_mem) (void)hipFree(d->skin_mem);
  d->skin_mem = nullptr;
  d->skin_vertices = 0;
  HK_HIP(hipMalloc(&d->skin_mem, n * (16 * 3 + 8)));
  d->bind_pos = (float4*)d->skin_mem;
  d->bind_nrm = d->bind_pos + n;
  d->weights = d->bind_nrm + n;
  d->joints = (uint2*)(d->weights + n);
  HK_HIP(hipMemcpy(d->bind_pos, bp.data(), n * 16, hipMemcpyHostToDevice));
  HK_HIP(hipMemcpy(d->bind_nrm, bn.data(), n * 16, hipMemcpyHostToDevice));
  HK_HIP(hipMemcpy(d->weights, w.data(), n * 16, hipMemcpyHostToDevice));
  HK_HIP(hipMemcpy(d->joints, j.data(), n * 8, hipMemcpyHostToDevice));
  d->skin_vertices = n_vertices;
  d->max_joint = max_joint;
  return HK_OK;
}

int hk_set_mesh_morph_targets(hk_ctx* c, const HkMeshIndex* mesh, uint32_t n_vertices, uint32_t n_targets, const float* base_positions, const float* base_normals,
                              const float* position_deltas, const float* normal_deltas) {
  HK_REQUIRE(c && mesh && base_positions && base_normals && position_deltas && n_vertices, HK_E_INVALID, "NULL argument or no vertices");
  HK_REQUIRE(n_targets >= 1 && n_targets <= HK_MORPH_MAX_TARGETS, HK_E_INVALID, "a morph set has between 1 and %u targets, not %u", HK_MORPH_MAX_TARGETS, n_targets);
  DeformMesh* d = nullptr;
  int rc;
  if ((rc = begin(c, mesh, &d))) return rc;
  HK_REQUIRE(n_vertices >= d->min_vertices && n_vertices <= d->max_vertices, HK_E_INVALID, "the mesh has between %u and %u vertices, not %u", d->min_vertices,
             d->max_vertices, n_vertices);
  const auto al = al256;
  const size_t plane = (size_t)n_vertices * 12, deltas = plane * n_targets;
  const size_t bytes = 2 * al(plane) + (normal_deltas ? 2 : 1) * al(deltas) + al((size_t)n_targets * 4) + al(((size_t)n_targets + 1) * 4);
  if ((rc = sync_all(c))) return rc;  // (a set given again: the kernels enqueued so far may still read the old one)
  if (d->morph_mem) (void)hipFree(d->morph_mem);
  d->morph_mem = nullptr;
  d->morph_vertices = d->morph_targets = 0;
  if (hipMalloc(&d->morph_mem, bytes) != hipSuccess) {
    (void)hipGetLastError();
    d->morph_mem = nullptr;
    HK_REQUIRE(false, HK_E_NOMEM, "device allocation of %zu bytes failed", bytes);
  }
  Carve cv{(uint8_t*)d->morph_mem};
  d->morph_base_p = cv.take<float>(plane);
  d->morph_base_n = cv.take<float>(plane);
  d->morph_dp = cv.take<float>(deltas);
  d->morph_dn = normal_deltas ? cv.take<float>(deltas) : nullptr;
  d->morph_w = cv.take<float>((size_t)n_targets * 4);
  d->morph_active = cv.take<uint32_t>(((size_t)n_targets + 1) * 4);
  HK_HIP(hipMemcpy(d->morph_base_p, base_positions, plane, hipMemcpyHostToDevice));
  HK_HIP(hipMemcpy(d->morph_base_n, base_normals, plane, hipMemcpyHostToDevice));
  HK_HIP(hipMemcpy(d->morph_dp, position_deltas, deltas, hipMemcpyHostToDevice));
  if (normal_deltas) HK_HIP(hipMemcpy(d->morph_dn, normal_deltas, deltas, hipMemcpyHostToDevice));
  d->morph_vertices = n_vertices;
  d->morph_targets = n_targets;
  return HK_OK;
}

int hk_skin_mesh(hk_ctx* c, const HkMeshIndex* mesh, const float* joint_matrices, uint32_t n_joints) {
  if (c) c->scene_epoch += 1;   // (scene memory is written: hk_context.hpp, primary-ray pipelining)
  HK_REQUIRE(c && mesh && joint_matrices && n_joints, HK_E_INVALID, "NULL argument or no joints");
  DeformMesh* d = lookup(c, *mesh);
  HK_REQUIRE(d && d->skin_vertices, HK_E_INVALID, "no skin set for this mesh (hk_set_mesh_skin)");
  HK_REQUIRE(d->max_joint < n_joints, HK_E_INVALID, "the skin names joint %u but only %u joint matrices were given", d->max_joint, n_joints);
  int rc;
  if ((rc = begin(c, mesh, &d))) return rc;
  if (n_joints > d->joint_cap && (rc = regrow(c, d->joint_mats, d->joint_cap, n_joints, 64))) return rc;
  uint8_t* st = nullptr;
  int k = 0;
  if ((rc = stage(c, (size_t)n_joints * 64, &st, &k))) return rc;
  memcpy(st, joint_matrices, (size_t)n_joints * 64);
  d->n_vertices = d->skin_vertices;
  return deform(c, d, k, [&](float4* vn) {
    motion_swap(d);
    launch_copy_region(c->stream, d->joint_mats, st, (size_t)n_joints * 64);  // (a copy kernel: the matrices are read per vertex)
    launch_mesh_skin(c->stream, d->bind_pos, d->bind_nrm, d->joints, d->weights, d->joint_mats, d->skin_vertices, d->pos, vn, d->box);
  });
}

int hk_deform_meshes(hk_ctx* c, const HkMeshDeform* items, uint32_t n) {
  HK_REQUIRE(c, HK_E_INVALID, "NULL context");
  if (n == 0) return HK_OK;
  HK_REQUIRE(items, HK_E_INVALID, "NULL items");
  std::vector<HkMeshDeformDevice> wide(n);  // (host pointers in the device item's fields, strides and flags zero: deform_batch stages what they name)
  for (uint32_t i = 0; i < n; ++i) {
    wide[i].mesh = items[i].mesh;
    wide[i].kind = items[i].kind;
    wide[i].count = items[i].count;
    wide[i].data = items[i].data;
    wide[i].normals = items[i].normals;
  }
  return deform_batch(c, wide.data(), n, false, nullptr);
}

int hk_deform_meshes_device(hk_ctx* c, const HkMeshDeformDevice* items, uint32_t n, void* producer_stream) {
  HK_REQUIRE(c, HK_E_INVALID, "NULL context");
  if (n == 0) return HK_OK;
  HK_REQUIRE(items, HK_E_INVALID, "NULL items");
  return deform_batch(c, items, n, true, (hipStream_t)producer_stream);
}

// Motion vectors for one mesh, on or off (hikari_hip.h).  Enabling gives the mesh its second plane and fills the current one from the
// triangle planes (DeformMesh::pos holds nothing before a mesh's first update): previous = current, no motion until a deformation.
// Disabling brings `pos` back to the plane inside the mesh's own allocation and frees the other behind an event.
int hk_set_mesh_motion_vectors(hk_ctx* c, const HkMeshIndex* mesh, uint32_t enable) {
  HK_REQUIRE(c && mesh, HK_E_INVALID, "NULL argument");
  DeformMesh* d = nullptr;
  int rc;
  if ((rc = begin(c, mesh, &d))) return rc;
  if ((enable != 0) == d->motion) return HK_OK;
  const size_t bytes = (size_t)d->max_vertices * 16;
  if (enable) {
    void* plane = nullptr;
    if (hipMalloc(&plane, bytes) != hipSuccess) {
      (void)hipGetLastError();
      HK_REQUIRE(false, HK_E_NOMEM, "device allocation of %zu bytes failed", bytes);
    }
    if ((rc = join_all(c))) { (void)hipFree(plane); return rc; }
    d->motion_mem = plane;
    d->pos_prev = (float4*)plane;
    const uint8_t* sbase = c->scene_mem + (c->two_slots ? 2 : 1) * c->dyn_capacity;
    const uint32_t p0 = d->mesh.primitive;
    launch_mesh_previous_fill(c->stream, (const float4*)(sbase + c->mesh.v0) + p0, (const float4*)(sbase + c->mesh.v1) + p0, (const float4*)(sbase + c->mesh.v2) + p0, d->n_tris,
                              d->pos, d->max_vertices);
    HK_HIP(hipGetLastError());
    d->motion = true;
    d->motion_dirty = d->motion_live = false;
    c->mv_enabled += 1;
  } else {
    if ((rc = join_all(c))) return rc;
    if (d->pos != d->pos_home) {  // (the current positions live in the plane that goes: read_mesh_geometry and the next refit find them at home)
      HK_HIP(hipMemcpyAsync(d->pos_home, d->pos, bytes, hipMemcpyDeviceToDevice, c->stream));
      d->pos = d->pos_home;
    }
    hipEvent_t done = nullptr;
    HK_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    HK_HIP(hipEventRecord(done, c->stream));
    retire(c, d->motion_mem, done);
    d->motion_mem = nullptr;
    d->pos_prev = nullptr;
    c->mv_enabled -= 1;
    c->mv_live -= d->motion_live ? 1u : 0u;
    d->motion = d->motion_dirty = d->motion_live = false;
  }
  c->scene_epoch += 1;  // (the live set may change: the next primary rays take the serial order, behind the table's rewrite)
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): launches of the motion pass in the last frame, meshes live in it, pixels it rewrote (counted only with
// HK_DEBUG_OPT_MOTION_COUNT set before the frame; waits for the frame)
int hk_debug_last_motion(hk_ctx* c, uint32_t out[3]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  out[0] = c->last_motion[0];
  out[1] = c->last_motion[1];
  out[2] = 0;
  if (c->mv_count && c->mv_counter && c->last_motion[0]) {
    HK_HIP(hipSetDevice(c->device));
    int rc;
    if ((rc = sync_all(c))) return rc;
    unsigned int v = 0;
    HK_HIP(hipMemcpy(&v, c->mv_counter, sizeof(v), hipMemcpyDeviceToHost));
    out[2] = v;
  }
  return HK_OK;
}

// Test hook (hikari_hip_debug.h)
int hk_debug_last_deform(hk_ctx* c, uint32_t out[6]) {
  HK_REQUIRE(c && out, HK_E_INVALID, "NULL argument");
  for (int k = 0; k < 6; ++k) out[k] = c->last_deform[k];
  return HK_OK;
}

// A new tree over the current triangles of one mesh, in place (hikari_hip.h).  The build is the instance level's (kernels_tree.hip
// launch_tree_build) fed from the mesh's triangle boxes; its topology replaces the one the refit climbs.  The mesh box and the triangle
// order stay, so nothing at the instance level moves: no propagation, only the staleness a deformation brings.
int hk_rebuild_mesh_tree(hk_ctx* c, const HkMeshIndex* mesh, uint32_t mode) {
  HK_REQUIRE(c && mesh, HK_E_INVALID, "NULL argument");
  HK_REQUIRE(mode == HK_TREE_SAH || mode == HK_TREE_LBVH, HK_E_INVALID, "unknown tree build mode %u", mode);
  HK_REQUIRE(c->have_meshes && c->have_materials && c->have_instances, HK_E_NOT_READY, "hk_upload_scene must come first");
  {  // the size limit holds for an UPLOADED mesh record, before anything is allocated for it (find_mesh repeats the first check)
    bool known = false;
    for (const HkInstance& in : c->instances) known = known || memcmp(&in.mesh, mesh, sizeof(HkMeshIndex)) == 0;
    HK_REQUIRE(known, HK_E_INVALID, "no uploaded instance carries the mesh record (%u, %u, %u, %u)", mesh->vertex, mesh->primitive, mesh->node_offset, mesh->node_count);
    HK_REQUIRE((mesh->node_count + 2) / 3 <= HK_MESH_REBUILD_MAX_TRIANGLES, HK_E_UNSUPPORTED, "a mesh of %u triangles is beyond the %u the device build takes",
               (mesh->node_count + 2) / 3, HK_MESH_REBUILD_MAX_TRIANGLES);
  }
  DeformMesh* d = nullptr;
  int rc;
  if ((rc = begin(c, mesh, &d))) return rc;
  const uint32_t n = d->n_tris;
  const size_t need = lbvh_scratch_bytes(n);
  if (need > c->lbvh_scratch_cap && (rc = regrow(c, c->lbvh_scratch, c->lbvh_scratch_cap, need + need / 4, 1))) return rc;
  if ((rc = join_all(c))) return rc;  // (the mesh-level region has one copy: behind every frame enqueued so far, as a deformation)
  c->scene_epoch += 1;                // (scene memory is written from here on: hk_context.hpp, primary-ray pipelining)
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  uint8_t* sbase = c->scene_mem + slots;
  if (!d->have_boxes) {
    const uint32_t p0 = d->mesh.primitive;
    launch_mesh_triangle_boxes(c->stream, (const float4*)(sbase + c->mesh.v0) + p0, (const float4*)(sbase + c->mesh.v1) + p0, (const float4*)(sbase + c->mesh.v2) + p0, n,
                               d->tree.tri_lo, d->tree.tri_hi);
    d->have_boxes = true;
  }
  float4* lo = (float4*)(sbase + c->mesh.nodes) + 2 * (size_t)d->mesh.node_offset;
  TreeBuild build;  // over the mesh's triangle boxes, into its node range of every ordering; the refit's topology is replaced
  build.mode = mode == HK_TREE_SAH ? 1 : 0;
  build.n = n;
  build.box_lo = d->tree.tri_lo; build.box_hi = d->tree.tri_hi;
  build.lo = lo; build.hi = lo + 1; build.stride = 2u;
  build.orderings = c->threaded ? 8u : 1u; build.ord_stride = 2 * c->mesh.node_cap;
  build.mesh_tree = true; build.keep = &d->tree;
  build.one_workgroup_top = c->mesh_rebuild_one_workgroup;
  build.scratch = c->lbvh_scratch;
  HK_REQUIRE(launch_tree_build(c->stream, build) == 0, HK_E_HIP, "device build of the mesh tree failed: %s", hipGetErrorString(hipGetLastError()));
  mark_deformed(c, {std::make_pair(d->mesh.node_offset, d->mesh.node_count)});
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): the emitter records and the alias table of the slot in use
int hk_debug_read_emitters(hk_ctx* c, float* records, uint32_t records_cap, uint32_t* n_records, float* alias, uint32_t alias_cap, uint32_t* n_alias) {
  HK_REQUIRE(c && n_records && n_alias, HK_E_INVALID, "NULL argument");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = flush_deform(c))) return rc;
  if ((rc = sync_all(c))) return rc;
  const uint32_t ne = (uint32_t)c->emissives.size(), na = (uint32_t)c->alias_table.size();
  *n_records = ne;
  *n_alias = na;
  if (!records && !alias) return HK_OK;
  HK_REQUIRE(records && alias && records_cap >= ne && alias_cap >= na, HK_E_INVALID, "need room for %u records and %u alias entries", ne, na);
  const uint8_t* base = c->scene_mem + (size_t)c->slot * c->dyn_capacity;
  std::vector<DEmissive> de(ne);
  if (ne) HK_HIP(hipMemcpy(de.data(), base + c->dyn_off.emissives, (size_t)ne * sizeof(DEmissive), hipMemcpyDeviceToHost));
  for (uint32_t e = 0; e < ne; ++e) {
    float* r = records + 8 * (size_t)e;
    r[0] = de[e].position_radius.x; r[1] = de[e].position_radius.y; r[2] = de[e].position_radius.z; r[3] = de[e].position_radius.w;
    r[4] = de[e].surface_area;
    memcpy(r + 5, &de[e].instance, 4); memcpy(r + 6, &de[e].alias_offset, 4); memcpy(r + 7, &de[e].alias_count, 4);
  }
  if (na) HK_HIP(hipMemcpy(alias, base + c->dyn_off.alias, (size_t)na * 8, hipMemcpyDeviceToHost));
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): the mesh-level node array, every ordering
int hk_debug_read_mesh_nodes(hk_ctx* c, HkNode* out, uint32_t cap, uint32_t* count, uint32_t* orderings) {
  HK_REQUIRE(c && (out || !cap), HK_E_INVALID, "NULL argument");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  if ((rc = sync_all(c))) return rc;
  const uint32_t n = (uint32_t)c->asset_nodes.size(), o = c->threaded ? 8u : 1u;
  if (count) *count = n;
  if (orderings) *orderings = o;
  if (!out) return HK_OK;
  HK_REQUIRE(cap >= n * o, HK_E_INVALID, "need room for %u nodes", n * o);
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  static_assert(sizeof(HkNode) == 32, "HkNode is two float4");
  for (uint32_t k = 0; k < o; ++k)  // (the orderings lie one node CAPACITY apart: hk_add_meshes)
    HK_HIP(hipMemcpy(out + (size_t)k * n, c->scene_mem + slots + c->mesh.nodes + (size_t)k * c->mesh.node_cap * 32, (size_t)n * 32, hipMemcpyDeviceToHost));
  return HK_OK;
}

// Test hook (hikari_hip_debug.h): the geometry of one deformed mesh as the device holds it (reads only)
int hk_debug_read_mesh_geometry(hk_ctx* c, const HkMeshIndex* mesh, float* positions, float* normals, uint32_t vertex_cap, float* triangles, uint32_t triangle_cap,
                                float* box, uint32_t* n_vertices, uint32_t* n_triangles) {
  HK_REQUIRE(c && mesh && n_vertices && n_triangles, HK_E_INVALID, "NULL argument");
  HK_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = finalize_scene(c))) return rc;
  DeformMesh* d = lookup(c, *mesh);
  if (!(d && d->deformed)) {  // never deformed here: what the planes hold for the mesh as the host's mirror describes it
    HK_REQUIRE(mesh->node_count >= 1 && (mesh->node_count + 2) % 3 == 0, HK_E_INVALID, "the mesh record names a tree of %u nodes", mesh->node_count);
    const uint32_t nt = (mesh->node_count + 2) / 3;
    HK_REQUIRE((size_t)mesh->primitive + nt <= c->primitives.size() && (size_t)mesh->node_offset + mesh->node_count <= c->asset_nodes.size() &&
                   mesh->vertex < c->vertices.size(),
               HK_E_INVALID, "the mesh record lies outside the uploaded mesh arrays");
    uint32_t nv = 0;
    for (uint32_t t = 0; t < nt; ++t)
      for (int k = 0; k < 3; ++k) nv = std::max(nv, c->primitives[mesh->primitive + t].vertices[k].index + 1u);
    HK_REQUIRE((size_t)mesh->vertex + nv <= c->vertices.size(), HK_E_INVALID, "the mesh's triangles name vertices beyond the uploaded ones");
    if ((rc = sync_all(c))) return rc;
    *n_vertices = nv;
    *n_triangles = nt;
    if (!positions && !normals && !triangles && !box) return HK_OK;
    HK_REQUIRE(positions && normals && triangles && box && vertex_cap >= nv && triangle_cap >= nt, HK_E_INVALID, "need room for %u vertices and %u triangles", nv, nt);
    const uint8_t* sbase = c->scene_mem + (c->two_slots ? 2 : 1) * c->dyn_capacity;
    HK_HIP(hipMemcpy(normals, (const float4*)(sbase + c->mesh.vn) + mesh->vertex, (size_t)nv * 16, hipMemcpyDeviceToHost));
    std::vector<float4> plane(nt);
    const size_t planes[3] = {c->mesh.v0, c->mesh.v1, c->mesh.v2};
    memset(positions, 0, (size_t)nv * 16);
    for (int k = 0; k < 3; ++k) {
      HK_HIP(hipMemcpy(plane.data(), (const float4*)(sbase + planes[k]) + mesh->primitive, (size_t)nt * 16, hipMemcpyDeviceToHost));
      for (uint32_t t = 0; t < nt; ++t) {
        memcpy(triangles + 12 * (size_t)t + 4 * k, &plane[t], 16);
        uint32_t index;
        memcpy(&index, &plane[t].w, 4);
        if (index < nv) {
          const float p[4] = {plane[t].x, plane[t].y, plane[t].z, 0.0f};
          memcpy(positions + 4 * (size_t)index, p, 16);
        }
      }
    }
    for (int k = 0; k < 3; ++k) { box[k] = INFINITY; box[3 + k] = -INFINITY; }
    for (uint32_t t = 0; t < nt; ++t)
      for (int v = 0; v < 3; ++v)
        for (int k = 0; k < 3; ++k) {
          box[k] = hmin(box[k], triangles[12 * (size_t)t + 4 * v + k]);
          box[3 + k] = hmax(box[3 + k], triangles[12 * (size_t)t + 4 * v + k]);
        }
    return HK_OK;
  }
  if ((rc = flush_deform(c))) return rc;
  if ((rc = sync_all(c))) return rc;
  const uint32_t nv = d->n_vertices, nt = d->n_tris;
  *n_vertices = nv;
  *n_triangles = nt;
  if (!positions && !normals && !triangles && !box) return HK_OK;
  HK_REQUIRE(positions && normals && triangles && box && vertex_cap >= nv && triangle_cap >= nt, HK_E_INVALID, "need room for %u vertices and %u triangles", nv, nt);
  const size_t slots = (c->two_slots ? 2 : 1) * c->dyn_capacity;
  const uint8_t* sbase = c->scene_mem + slots;
  HK_HIP(hipMemcpy(positions, d->pos, (size_t)nv * 16, hipMemcpyDeviceToHost));
  HK_HIP(hipMemcpy(normals, (const float4*)(sbase + c->mesh.vn) + d->mesh.vertex, (size_t)nv * 16, hipMemcpyDeviceToHost));
  std::vector<float4> plane(nt);
  const size_t planes[3] = {c->mesh.v0, c->mesh.v1, c->mesh.v2};
  for (int k = 0; k < 3; ++k) {
    HK_HIP(hipMemcpy(plane.data(), (const float4*)(sbase + planes[k]) + d->mesh.primitive, (size_t)nt * 16, hipMemcpyDeviceToHost));
    for (uint32_t t = 0; t < nt; ++t) memcpy(triangles + 12 * (size_t)t + 4 * k, &plane[t], 16);
  }
  uint32_t words[6];
  HK_HIP(hipMemcpy(words, d->box, sizeof(words), hipMemcpyDeviceToHost));
  for (int k = 0; k < 6; ++k) {  // (kernels_deform.hip box_word, inverted)
    const uint32_t u = (words[k] & 0x80000000u) ? (words[k] & 0x7FFFFFFFu) : ~words[k];
    memcpy(box + k, &u, 4);
  }
  return HK_OK;
}

}  // extern "C"
