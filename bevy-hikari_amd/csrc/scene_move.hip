// scene_move.hip - a loaded scene moved to a new allocation (hk_context.hpp SceneMove; DESIGN 3 "Meshes that arrive later").  An edit that
// outgrows or leaves the scene's allocation - meshes added, meshes removed, instance slots grown - fills a new one device to device behind
// every frame enqueued so far; frames in flight go on reading the old one.  The callers differ in WHAT they enqueue, in nothing else.
#include "hk_context.hpp"

namespace hk {
void retire(hk_ctx* c, void* p, hipEvent_t done) { c->retired.push_back(hk_ctx::Retired{p, done}); }
// hipFree may wait for the device by itself: this is called only where the context has just waited for its streams anyway (sync_all, the
// wait of build_on_device, hk_destroy), never on the per-frame path - until then a retired allocation merely stays allocated
void poll_retired(hk_ctx* c, bool wait) {
  size_t kept = 0;
  for (const hk_ctx::Retired& r : c->retired) {
    if (!wait && hipEventQuery(r.done) != hipSuccess) {
      c->retired[kept++] = r;
      continue;
    }
    (void)hipFree(r.p);
    (void)hipEventDestroy(r.done);
  }
  c->retired.resize(kept);
}
MeshSizes move_room(const MeshSizes& need) {
  auto room = [](size_t n, size_t unit) { return ((3 * n + 1) / 2 + unit - 1) / unit * unit; };
  return MeshSizes{room(need.nodes, 1), room(need.prims, 4), room(need.verts, 4)};
}
// Exits: HK_OK - `m` holds mem, three (with `extra` four) events, wide / rank / extra where asked for, the ranks' fill is enqueued;
// HK_E_HIP - what had been made is freed again (a fill that was refused is not enqueued), `m` is empty
int move_begin(const hk_ctx* c, const MeshSizes& caps, size_t dyn_capacity, bool with_wide, bool with_rank, size_t extra_bytes, const char* refusal, SceneMove* m) {
  *m = SceneMove{};
  m->mesh = mesh_region_layout(caps, c->threaded ? 8u : 1u);
  m->dyn_capacity = dyn_capacity;
  bool ok = hipMalloc((void**)&m->mem, 2 * dyn_capacity + m->mesh.bytes) == hipSuccess;
  if (ok && extra_bytes) ok = hipMalloc((void**)&m->extra, extra_bytes) == hipSuccess;
  for (int k = 0; k < (extra_bytes ? 4 : 3) && ok; ++k) ok = hipEventCreateWithFlags(&m->done[k], hipEventDisableTiming) == hipSuccess;
  if (ok && with_wide) ok = hipMalloc((void**)&m->wide, caps.nodes * 128) == hipSuccess;
  if (ok && with_rank) ok = hipMalloc((void**)&m->rank, caps.prims * 4) == hipSuccess && hipMemsetAsync(m->rank, 0xFF, caps.prims * 4, c->stream) == hipSuccess;
  if (ok) return HK_OK;
  const hipError_t e = hipGetLastError();
  move_abort(c, m, false);
  set_error("%s: %s", refusal, hipGetErrorString(e));
  return HK_E_HIP;
}

// What moves: every ordering's node plane with the old and the new stride, the triangle and vertex planes, then wide records and ranks
uint32_t move_planes(const hk_ctx* c, const SceneMove& m, MovePlane out[HK_MOVE_PLANES]) {
  const MeshRegion &a = c->mesh, &b = m.mesh;
  const uint8_t* from = c->scene_mem + 2 * c->dyn_capacity;
  uint8_t* to = m.mem + 2 * m.dyn_capacity;
  uint32_t n = 0;
  for (size_t o = 0; o < (c->threaded ? 8u : 1u); ++o) out[n++] = MovePlane{from + a.nodes + o * a.node_cap * 32, to + b.nodes + o * b.node_cap * 32, 0u, 5u, a.node_cap, b.node_cap};
  for (size_t MeshRegion::*v : {&MeshRegion::v0, &MeshRegion::v1, &MeshRegion::v2}) out[n++] = MovePlane{from + a.*v, to + b.*v, 1u, 4u, a.prim_cap, b.prim_cap};
  out[n++] = MovePlane{from + a.vn, to + b.vn, 2u, 4u, a.vert_cap, b.vert_cap};
  out[n++] = MovePlane{from + a.vuv, to + b.vuv, 2u, 3u, a.vert_cap, b.vert_cap};
  if (m.wide) out[n++] = MovePlane{(const uint8_t*)c->wide_blas, (uint8_t*)m.wide, 0u, 7u, c->wide_blas_slots, b.node_cap};
  if (m.rank) out[n++] = MovePlane{(const uint8_t*)c->wide_blas_rank, (uint8_t*)m.rank, 1u, 2u, c->wide_rank_primitives, b.prim_cap};
  return n;
}

// Exit: nothing of `m` is left, the context unchanged.  `enqueued`: the stream is waited for first - what may be enqueued must not outlive its targets
void move_abort(const hk_ctx* c, SceneMove* m, bool enqueued) {
  if (enqueued) (void)hipStreamSynchronize(c->stream);
  for (void* q : {(void*)m->mem, (void*)m->wide, (void*)m->rank, (void*)m->extra}) (void)hipFree(q);  // (NULL: nothing)
  for (hipEvent_t e : m->done)
    if (e) (void)hipEventDestroy(e);
  *m = SceneMove{};
}
// The switch: frames enqueued from here on read the new allocation, the ones in flight the old one until `done`.  Exits: HK_E_HIP - an event
// was not recorded: move_abort behind a wait; HK_OK - what was replaced, and `extra`, is retired with its event, the other events are destroyed
int move_commit(hk_ctx* c, SceneMove* m, int slot) {
  bool ok = true;
  for (int k = 0; k < 4 && ok; ++k) ok = !m->done[k] || hipEventRecord(m->done[k], c->stream) == hipSuccess;
  if (!ok) {
    const hipError_t e = hipGetLastError();
    move_abort(c, m, true);
    set_error("the move of the scene failed: %s", hipGetErrorString(e));
    return HK_E_HIP;
  }
  retire(c, c->scene_mem, m->done[0]);
  if (m->wide) { retire(c, c->wide_blas, m->done[1]); c->wide_blas = m->wide; c->wide_blas_slots = m->mesh.node_cap; }
  else (void)hipEventDestroy(m->done[1]);
  if (m->rank) { retire(c, c->wide_blas_rank, m->done[2]); c->wide_blas_rank = m->rank; c->wide_rank_primitives = m->mesh.prim_cap; }
  else (void)hipEventDestroy(m->done[2]);
  if (m->extra) retire(c, m->extra, m->done[3]);
  c->scene_mem = m->mem;
  c->dyn_capacity = m->dyn_capacity;
  c->mesh = m->mesh;
  c->slot = slot;
  repoint_scene(c);
  *m = SceneMove{};
  return HK_OK;
}
}  // namespace hk
