// hk_context.hpp - the context behind the C ABI (private to libhikari_hip.so): `struct hk_ctx` and what the translation units that
// work on it share.
//   context.hip       lifetime, screen-space resources, the frame graph (hk_frame_*, hk_pass_run), bands, buffers, statistics
//   scene_layout.hip  uploads and the layout conversion: reference-layout scene arrays -> the device's scene blob (finalize_scene)
//   scene_refit.hip   instance motion and instance-set changes on the device (hk_refit_scene_instances, hk_rebuild_scene_trees, ...)
//   scene_load.hip    mesh trees built on the device at scene load (hk_load_scene); scene_append.hip: meshes appended later (hk_add_meshes);
//                     scene_remove.hip: meshes removed, the mesh level compacted (hk_remove_meshes)
//   scene_move.hip    the scene moved to a new allocation in stream order, for the edits above and below (move_begin ... move_commit, retire)
//   scene_instances.hip  the instance set changed from device state: after deformations and device poses (hk_change_scene_instances)
//   probes.hip        measurement hooks (hk_measure_*, hk_debug_math)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <iterator>
#include <chrono>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "hk_internal.hpp"
#include "hk_kernels.hpp"

#define HK_HIP(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      ::hk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return HK_E_HIP;                                                                   \
    }                                                                                    \
  } while (0)

using namespace hk;   // (a private header: every translation unit that includes it works inside these two namespaces)
using namespace hkd;

namespace hk {

template <typename T>
struct DevArray {
  T* p = nullptr;
  size_t n = 0;
  int upload(const std::vector<T>& h) {
    if (p) { (void)hipFree(p); p = nullptr; }
    n = h.size();
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HK_HIP(hipMalloc((void**)&p, bytes));
    if (n) HK_HIP(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    return HK_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// One device allocation for all scene arrays, each 16-B aligned.
struct Blob {
  std::vector<uint8_t> bytes;
  template <typename T>
  size_t add(const std::vector<T>& v) {
    size_t off = (bytes.size() + 15) & ~(size_t)15;
    bytes.resize(off + std::max<size_t>(v.size(), 1) * sizeof(T), 0);
    if (!v.empty()) memcpy(bytes.data() + off, v.data(), v.size() * sizeof(T));
    return off;
  }
};

struct TimedLaunch {
  uint32_t slot;
  hipEvent_t start, stop;
};

// IEEE minNum / maxNum with -0 < +0 (the numeric contract of hk_device_math.hpp) on the host
inline float hmin(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? a : b;
  return a < b ? a : b;
}
inline float hmax(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? b : a;
  return a > b ? a : b;
}
inline uint32_t hash_u32(uint32_t value) {  // utils.wgsl:15-24
  uint32_t state = value;
  state = state ^ 2747636419u;
  state = state * 2654435769u;
  state = state ^ (state >> 16u);
  state = state * 2654435769u;
  state = state ^ (state >> 16u);
  state = state * 2654435769u;
  return state;
}
inline float as_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// a material as the device holds it: four float4 (base colour, emissive, roughness / metallic / reflectance, the four texture ids)
inline void material_rows(const HkMaterial& m, float4 rows[4]) {
  rows[0] = make_float4(m.base_color[0], m.base_color[1], m.base_color[2], m.base_color[3]);
  rows[1] = make_float4(m.emissive[0], m.emissive[1], m.emissive[2], m.emissive[3]);
  rows[2] = make_float4(m.perceptual_roughness, m.metallic, m.reflectance, 0.0f);
  rows[3] = make_float4(as_f(m.base_color_texture), as_f(m.emissive_texture), as_f(m.metallic_roughness_texture), as_f(m.occlusion_texture));
}

}  // namespace hk


// byte offsets of the arrays inside the instance-level region of the scene allocation
struct DynOffsets { size_t tlas, instances, prev_models, light_lo, light_hi, emissives, alias, materials, tex_info, srgb_lut, flat; uint32_t flat_count, flat_orderings; };

struct MeshSizes { size_t nodes, prims, verts; };   // sizes or capacities of the mesh-level lists, in elements (nodes: per ordering)
// The mesh-level region of the scene allocation (mesh_region_layout).  Its sub-arrays keep CAPACITIES behind their contents: nodes per ordering
// - the stride between two orderings, DScene::blas_stride - primitives, vertices.  A host layout leaves them equal to the mirrors' sizes; an
// edit that does not fit moves the scene (scene_move.hip).
struct MeshRegion {
  size_t node_cap = 0, prim_cap = 0, vert_cap = 0;
  size_t nodes = 0, v0 = 0, v1 = 0, v2 = 0, vn = 0, vuv = 0;  // byte offsets of the sub-arrays inside the region
  size_t bytes = 0;                                           // of the region (covers the capacities)
};

struct hk_ctx {
  int device = 0;
  uint32_t flags = 0;
  hipStream_t stream = nullptr;      // stream all work is enqueued on (own_stream unless hk_set_stream)
  hipStream_t own_stream = nullptr;
  bool own_stream_high = false;      // ... created at the device's highest stream priority (context.hip pick_main_stream)
  bool main_priority_decided = false; // ... by the rule, at the first hk_resize
  // Primary-ray pipelining (round 6; context.hip stage TEMPORAL): frame n's primary rays on a stream of their own, ordered only behind
  // what last touched the G-buffer planes of ITS parity - frame n - 2, whose post-processing event covers all three of that frame's
  // streams - so that they run beside frame n - 1's spatial pass instead of behind it.  The stream exists only where the main stream
  // sits in the high-priority queue pool (a fourth stream of the default priority then has a hardware queue to itself).  scene_epoch
  // counts every write to scene memory (uploads, refits, rebuilds: scene_layout.hip / scene_refit.hip); a frame whose scene was
  // written since the last one takes the serial order - those writes sit behind the previous frame's spatial pass on the main stream.
  hipStream_t pre_stream = nullptr;
  hipEvent_t pre_done = nullptr, pre_scene_mark = nullptr;   // pre_scene_mark: the main stream behind the latest writes to scene memory
  bool pre_scene_marked = false;
  int prepass_pipeline = -1;          // HK_DEBUG_OPT_PREPASS_PIPELINE: -1 the rule, 0 never, 1 whenever the order allows
  uint64_t scene_epoch = 0, pre_seen_epoch = 0;
  bool pre_chain_ok = false;          // the previous frame went through stage TEMPORAL with the other parity, without the AA tail
  uint32_t pre_last_parity = 0;
  uint64_t prepasses_pipelined = 0;
  int main_priority = -1;            // HK_DEBUG_OPT_MAIN_PRIORITY: -1 the rule, 0 default priority, 1 highest
  hipStream_t side_stream = nullptr;   // the direct-light dispatches of the frame path run here (unless HK_CTX_SINGLE_STREAM)
  hipEvent_t fork_event = nullptr, join_event = nullptr;
  bool forked = false;                 // side_stream holds work the main stream has not waited for yet
  // Round 6: the main stream no longer waits for the side stream at the end of a frame.  What reads the direct-light dispatches'
  // outputs is the post-processing (post stream: it waits for side_done itself); the NEXT frame's primary rays and indirect pass touch
  // nothing the direct-light dispatches of this frame read or write - the G-buffer planes are double-buffered by frame parity (normal
  // and instance_material included, below), the sun / emissive reservoirs are the side stream's own - so the side stream may run up
  // to the post-processing behind.  side_parity = the frame parity of the work it was last given (a frame of the SAME parity joins).
  hipEvent_t side_done = nullptr;
  // per frame parity: 0 = the side stream holds nothing of that parity the main stream has not been ordered behind, 1 = it does,
  // 2 = it does, and the post-processing of parity side_cover[.] waits for it (so waiting for THAT post-processing is enough)
  uint8_t side_state[2] = {0, 0};
  uint8_t side_cover[2] = {0, 0};
  void* normal_twin = nullptr;
  void* instance_material_twin = nullptr;
  // Frame pipelining (round 3; round 6: the whole post-processing).  Demodulation, the a-trous levels and tone mapping of frame n - and,
  // on a band with a communicator, the halo exchange B in front of them - run on a third stream, so that the main stream goes straight
  // on to frame n + 1's primary rays and light passes.  What both touch is double-buffered by frame parity: albedo, depth gradient, the
  // derived planes (dn_g, depth) the a-trous taps read, and (round 6) the render / variance planes the light passes write and
  // demodulation reads.  Stream order keeps the denoiser's own planes safe (post-processing n + 1 follows post-processing n); the main
  // stream waits for the post-processing of the LAST FRAME OF THE SAME PARITY before it writes that parity's planes again.
  hipStream_t post_stream = nullptr;
  hipEvent_t post_fork = nullptr;
  hipEvent_t post_done[2] = {nullptr, nullptr};  // post stream: end of the post-processing of the last frame of that parity
  bool post_pending[2] = {false, false};        // ... which the main stream has not waited for yet
  bool post_forked = false;                     // hk_frame_render moved the context to the post stream ahead of stage POST_PROCESS (exchange B goes there too)
  hipStream_t post_saved_main = nullptr;
  void* albedo_twin = nullptr;         // the planes of the OTHER frame parity (swapped with buf[HK_BUF_ALBEDO] ... in hk_frame_begin)
  void* depth_gradient_twin = nullptr;
  void* dn_g_twin = nullptr;
  void* render_twin[3] = {nullptr, nullptr, nullptr};
  void* variance_twin[3] = {nullptr, nullptr, nullptr};
  // test / measurement switches (hikari_hip_debug.h hk_debug_set_option; the library reads no environment variable)
  int spatial_window = -1;               // which form of k_spatial_reuse a launch takes: -1 by its size, 0 plain, 1 windowed (kernels.hip launch_spatial)
  uint64_t spatial_windowed_launches = 0;
  // the background's known records for the spatial passes (hk_kernels.hpp SpatialKnown): made before the context's first spatial launch
  // (context.hip spatial_known_table), handed to every spatial launch while the switch is on
  bool spatial_known_on = true;          // HK_DEBUG_OPT_SPATIAL_KNOWN
  hkd::SpatialKnown* spatial_known = nullptr;
  uint64_t spatial_known_launches = 0;   // spatial launches that were handed the table
  bool frame_pipeline = true;            // the a-trous levels of frame n beside frame n + 1's light passes (post_stream)
  bool wf_timeline = false;              // the instrumented twin of the trace kernels (tools/wf_timeline.py)
  bool flat_walk = true;                 // the one-level tree for scenes under one transform (scene_layout.hip)
  int flat_orderings = 0;                // ... with this many direction orderings (0: as many as fit 4 KB)
  bool trace_update = false;             // timings of scene updates on stderr
  bool in_frame_render = false;          // hk_frame_render is driving the stages (its internal frame flag is only valid then)

  // host copies of the reference-layout scene (kept for the layout conversion)
  std::vector<HkVertex> vertices;
  std::vector<HkPrimitive> primitives;
  std::vector<HkNode> asset_nodes;
  std::vector<HkMaterial> materials;
  std::vector<HkInstance> instances;
  std::vector<HkNode> instance_nodes;
  std::vector<HkEmissive> emissives;
  std::vector<HkNode> emissive_nodes;
  std::vector<HkAliasEntry> alias_table;
  struct HostTexture { std::vector<uint32_t> texels; uint32_t w, h, flags; };
  std::vector<HostTexture> textures;
  bool have_meshes = false, have_materials = false, have_instances = false, have_noise = false;
  // what finalize_scene has to redo: the mesh-level region, the instance-level region, the texel buffer
  bool mesh_dirty = true, dynamic_dirty = true, textures_dirty = true;
  std::vector<float> prev_models;          // PreviousMeshUniform::transform per instance (optional)
  std::vector<int64_t> node_prim_offset;   // primitive offset each BLAS node's leaves index (from the last mesh-level build)

  // device scene
  uint8_t* scene_mem = nullptr;  // every scene array in one allocation (so small scenes can be staged in LDS by one copy loop)
  size_t dyn_capacity = 0;
  MeshRegion mesh;               // the mesh-level region behind the slots
  // Scenes too big for the LDS copy keep TWO slots of the instance-level region, [slot 0][slot 1][mesh region]: an
  // instance-only update goes through pinned staging into the slot the frames in flight do NOT read, in stream
  // order, so neither the host nor the GPU waits (animated scenes must not stall on the host).
  bool two_slots = false;
  int slot = 0;
  Blob dyn_blob;                // the instance-level region as last laid out: kept so that a per-frame update re-uses warm pages
  std::vector<float4> tlas_tmp;  // (20 MB of fresh allocations per update cost more in page faults than the layout itself)
  bool trees_pending_on_device = false;  // hk_update_scene_instances: the trees about to be uploaded are stand-ins the device overwrites in
                                         // stream order - no point threading their orderings on the host
  bool threaded = false;  // eight direction-ordered flattenings of every TLAS / BLAS are stored (hikari_hip.h HK_CTX_EXACT_TRAVERSAL)
  uint8_t* staging[2] = {nullptr, nullptr};
  size_t staging_bytes[2] = {0, 0};
  hipEvent_t staging_done[2] = {nullptr, nullptr};
  bool staging_pending[2] = {false, false};
  uint64_t async_instance_uploads = 0;
  // What a move of the scene replaces (scene_move.hip) - or a grown build scratch - is freed once the event recorded behind the move has
  // passed, polled at later calls: frames in flight go on reading it.
  struct Retired { void* p; hipEvent_t done; };
  std::vector<Retired> retired;
  uint32_t last_add[5] = {0, 0, 0, 0, 0};   // hk_debug_last_add
  // hk_add_meshes_device (scene_append.hip): the device block its launch assembles the sources' records into - kept like the build scratch,
  // grown behind an event - the producer's stream before that launch and the launch before the producer, and what the last add took
  void* add_block = nullptr;
  size_t add_block_cap = 0;
  hipEvent_t add_src_ready = nullptr, add_src_read = nullptr;
  hipEvent_t add_ev[2] = {nullptr, nullptr};     // around that launch, made and recorded only while HK_DEBUG_OPT_ADD_SOURCE_TIMES is set (hk_debug_last_add_source_times)
  bool time_add_sources = false;
  uint32_t last_add_sources[4] = {0, 0, 0, 0};   // hk_debug_last_add_sources
  double last_add_source_ms[3] = {0, 0, 0};      // hk_debug_last_add_source_times
  double last_add_ms[4] = {0, 0, 0, 0};     // hk_debug_last_add_times
  uint64_t last_remove[6] = {0, 0, 0, 0, 0, 0};   // hk_debug_last_remove (scene_remove.hip)
  hipEvent_t rm_ev[2] = {nullptr, nullptr};       // around the compaction launch of the last hk_remove_meshes (hk_debug_last_remove_ms)
  bool rm_timed = false;
  uint64_t static_rebuilds = 0, dynamic_rebuilds = 0;
  // Parked previous_spatial stores (HK_CTX_DETERMINISTIC_SCATTER; every band of a sharded frame with a history halo: SURVEY 8e
  // step 6), one set per light channel.  `to` and the records are the HK_BUF_PARKED_* planes (c->buf: bands exchange their rows),
  // the winners are private.  Allocated on first use (ensure_parked).
  int* det_winner[3] = {nullptr, nullptr, nullptr};
  // Round 6: a single context resolves the reference's scatter race deterministically BY DEFAULT, in the light form (hk_kernels.hpp
  // LightTargets::det_lite) - for the channels whose previous_spatial buffer has a reader (the spatial pass that is on); with
  // HK_CTX_DETERMINISTIC_SCATTER for all three; HK_CTX_RACING_SCATTER restores the reference's race.  det_lite_clean[k]: channel k's
  // winner plane holds -1 everywhere (the light form hands it back that way; the full form of a band does not).
  bool det_lite_clean[3] = {false, false, false};
  // A temporal dispatch of PART of the rows (hk_pass_run with a row range, single context) cannot take the light form: whether a slot's
  // owner stores, and which parked store is the highest, is known only once every piece of the frame has run, in whatever order.  Such a
  // dispatch parks every store (the full form) and resolves over the WHOLE image after each piece, from the notes all pieces of the frame
  // have left so far.  pieces_new_frame[k]: channel k's notes are an earlier frame's (hk_frame_begin) or another form's - the first piece clears them.
  // Cost: every piece memsets the winner plane and runs k_join_winners + k_resolve_scatter over all rw * rh pixels - O(pieces x image), the
  // price of any order; the frame path never takes it.  Limitation: rows dispatched AGAIN within one frame replace their notes, but a store
  // that an earlier resolve of the same frame already landed in previous_spatial stays there even if the rows' new note no longer aims at
  // that slot - the pieces of a frame are meant to tile the image once; hk_frame_begin starts over.
  bool pieces_new_frame[3] = {true, true, true};
  // uniform-tile store elision (hk_kernels.hpp TileMeta): one record per 8x8 tile per reservoir buffer; tile_meta_zero[k] = the
  // device array of buffer k is known to be all zero ("contents unknown" everywhere)
  TileMeta* tile_meta[10] = {};
  bool tile_meta_zero[10] = {};
  int tiles_x = 0, tiles_y = 0;
  uint32_t elide_serial = 0;
  // Known results (DESIGN 4 "Empty tiles"): one byte per 8x8 tile and frame parity, written by the primary rays of hk_frame_stage - 1 where
  // every ray of the tile missed - and handed to the launches of the same frame that may skip the arithmetic leading to a known result
  // (context.hip known_empty_plane holds the rule).  empty_frame / lights_frame: the frame whose primary rays wrote the parity's plane /
  // whose three light passes ran over every row (demodulation's shortcut rests on the variance they wrote); *_ok = that entry holds.
  uint8_t* empty_tiles[2] = {nullptr, nullptr};
  bool empty_ok[2] = {false, false}, lights_ok[2] = {false, false};
  uint32_t empty_frame[2] = {0, 0}, lights_frame[2] = {0, 0};
  // Background stores (DESIGN 4 "Empty tiles"): a second byte per tile and parity, written by the same primary rays - the empty-tile byte
  // plus HK_TILE_KEPT where the tile was empty in the frame that last wrote the parity's physical planes too, whose byte the rays found
  // in empty_tiles.  Such a wave skips the stores that would rewrite the background's constants.  kept_ok: the plane was written by frame
  // kept_frame's primary rays (they skipped the G-buffer's stores); kept_lights: that earlier frame's light passes had stored their
  // constants too, so this frame's may skip variance / render (context.hip kept_grant, kept_plane_for_lights).  Cleared with empty_ok
  // by everything that clears it.
  uint8_t* kept_tiles[2] = {nullptr, nullptr};
  bool kept_ok[2] = {false, false}, kept_lights[2] = {false, false};
  uint32_t kept_frame[2] = {0, 0};
  // Post stores (DESIGN 4 "Empty tiles"; context.hip post_grant holds the rule).  The planes demodulation and the a-trous levels write are
  // NOT twinned by frame parity: what they hold is what the last post chain left, whichever frame's it was.  post_last describes that
  // chain - ok only if it ran through hk_frame_stage over every row with the empty-tile plane in all five launches; every later post
  // stage replaces it, everything that ends the other grants clears it.  The tone-mapped image IS twinned (hk_frame_begin): post_tone[p]
  // is the same record for the chain that last wrote parity p's physical plane.  empty_serial[p]: which TEMPORAL stage wrote
  // empty_tiles[p] (frame numbers may repeat).  post_kept / post_tone_kept: this parity's kept-tile plane carries HK_TILE_POST_KEPT,
  // formed against the post chain post_against / post_tone_against (PostRecord::id).
  struct PostRecord {
    bool ok = false;
    uint64_t id = 0;          // of the post stage that made it (post_counter)
    uint64_t serial = 0;      // empty_serial of the frame it belonged to
    uint32_t parity = 0, nch = 0;
    float clear[4] = {0, 0, 0, 0};
    const void* tone_plane = nullptr;   // the physical plane its level 3 wrote the tone-mapped image to
  };
  PostRecord post_last{}, post_tone[2]{};
  uint64_t stage_serial = 0, post_counter = 0, empty_serial[2] = {0, 0};
  bool post_kept[2] = {false, false}, post_tone_kept[2] = {false, false};
  uint64_t post_against[2] = {0, 0}, post_tone_against[2] = {0, 0};
  bool post_use = false, post_tone_use = false;   // for the five launches of the post stage that is running
  bool pre_last_pipelined = false;       // the last primary rays ran on the pre stream
  bool pixel_identity = false;           // at ratio 1 the kernels' coordinate chains map every pixel to itself (certify_pixel_identity, per hk_resize)
  bool host_wrote = false;               // hk_write_buffer since the last primary rays: the next frame keeps today's path
  bool in_frame_stage = false;           // hk_frame_stage is launching (hk_pass_run's hand-driven passes never get the plane)
  bool known_results = true;             // HK_DEBUG_OPT_KNOWN_RESULTS
  uint64_t empty_plane_launches = 0;     // launches that were handed the plane (hk_debug_empty_tiles)
  // ---- instance motion on the device (hk_refit_scene_instances, kernels_scene.hip)
  DynOffsets dyn_off{};                   // where the arrays of the instance-level region are (the slot in use)
  float4 *rf_inst_lo = nullptr, *rf_inst_hi = nullptr, *rf_prev_models = nullptr;  // world AABB / previous model per instance
  uint32_t* rf_emissive_of_instance = nullptr;
  float* rf_alias_scratch = nullptr;
  size_t rf_instances = 0, rf_alias = 0;  // sizes the side arrays were allocated for
  bool rf_ready = false;                  // side arrays describe the scene as uploaded (cleared by every host-side rebuild)
  hkd::RefitUpdate* rf_updates[2] = {nullptr, nullptr};  // pinned, read by the kernel over PCIe
  size_t rf_updates_cap[2] = {0, 0};
  hipEvent_t rf_done[2] = {nullptr, nullptr};
  bool rf_pending[2] = {false, false};
  int rf_k = 0;
  std::vector<uint32_t> rf_last_moved;    // instances whose `moved` flag is set on the device
  // material edits on the device (hk_update_materials): pinned records (the MaterialUpdate array, then the ids of the emitters to
  // re-derive), double-buffered against the kernels that read them like rf_updates
  uint8_t* mt_updates[2] = {nullptr, nullptr};
  size_t mt_updates_cap[2] = {0, 0};      // bytes
  hipEvent_t mt_done[2] = {nullptr, nullptr};
  bool mt_pending[2] = {false, false};
  int mt_k = 0;
  bool rf_motion_taken = false;           // a case-B material edit took the builder's poses along since the last frame: a refit that finds
                                          // no pose left to change has nothing to do (it would clear the `moved` flags of this frame's movers)
  bool mirrors_stale = false;             // the host copies of emissives / tree boxes no longer describe the device scene
  // mesh deformation (mesh_deform.hip): per deformable mesh its tree topology, refit planes and skin, created on first use and dropped by
  // hk_upload_meshes; a pool of pinned staging buffers for the vertex / joint data, each reused once the event after its last reader has
  // passed (a call never waits on the host: with none free it adds one)
  std::vector<struct DeformMesh*> deform;
  struct DeformStage { uint8_t* p = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; };
  std::vector<DeformStage> df_stage;
  hkd::RefitUpdate* df_records = nullptr; // device: the emitter records of one propagation, one per emitting instance of a deformed mesh
  size_t df_records_cap = 0;
  uint64_t df_batch = 0;                  // counts hk_deform_meshes calls (a mesh named twice in one batch carries the call's number already)
  uint32_t last_deform[6] = {0, 0, 0, 0, 0, 0};  // hk_debug_last_deform
  hipEvent_t df_src_ready = nullptr, df_src_read = nullptr;  // hk_deform_meshes_device: the producer's stream before the batch, the batch's vertex launch before the producer
  bool deform_pending = false;            // deformed meshes whose new boxes have not reached the instance level yet (flush_deform)
  bool meshes_deformed = false;           // a mesh was deformed on the device since the last hk_upload_meshes: its host copies are stale
  // motion vectors of deforming meshes (hk_set_mesh_motion_vectors, mesh_deform.hip).  A mesh that opted in owns two position
  // planes; it is LIVE in a frame if it was deformed since the frame before enqueued its primary rays.  mv_table: per instance the
  // previous-position plane of its mesh, or NULL - rewritten in stream order at the first primary rays of every frame with a live mesh.
  // mv_frame counts hk_frame_begin, mv_seen the frame whose primary rays last went through motion_frame (row pieces of one frame share it).
  hkd::MotionEntry* mv_table = nullptr;
  size_t mv_table_cap = 0;                // instances
  unsigned int* mv_counter = nullptr;     // pixels rewritten by the frame's motion passes (HK_DEBUG_OPT_MOTION_COUNT)
  bool mv_count = false;
  uint32_t mv_enabled = 0, mv_live = 0;   // meshes that opted in / that are live in the frame most recently begun
  uint64_t mv_frame = 0, mv_seen = 0;
  uint32_t last_motion[2] = {0, 0};       // hk_debug_last_motion: launches of the motion pass in the last frame, meshes live
  // poses from device memory (hk_set_instance_transforms_device, scene_refit.hip).  poses_on_device: the device's poses were last set
  // from memory the host never saw - instances[].model / min / max / inverse_transpose_model and prev_models no longer describe the
  // device (every reader of them asks; hk_upload_instances clears it).  pd_boxes: the mesh box of every instance (Aabb centre, half
  // extents; 2 float4) as the builder gave it, pd_boxes_host what it holds; pd_all: the record order of a call that names every instance
  // (instance, instance), emitters first, valid for the instance list pd_all_generation; pd_records: the call's RefitUpdate records.
  bool poses_on_device = false;
  float4* pd_boxes = nullptr;
  std::vector<float> pd_boxes_host;
  uint2* pd_all = nullptr;
  hkd::RefitUpdate* pd_records = nullptr;
  size_t pd_cap = 0;                      // instances the three were allocated for
  bool pd_all_ready = false;
  uint64_t pd_all_generation = 0;
  uint32_t pd_all_emitters = 0, pd_all_emitter_triangles = 0;
  hipEvent_t pd_src_ready = nullptr, pd_src_read = nullptr;  // the producer's stream before the call's launches, the pose kernel before the producer
  uint32_t last_instance_change[4] = {0, 0, 0, 0};  // hk_debug_last_instance_change (scene_instances.hip)
  uint32_t last_pose[2] = {0, 0};         // hk_debug_last_pose: launches of the last call, 1 if it copied mesh boxes to the device
  uint64_t instances_generation = 0;      // counts hk_upload_instances (the instance lists of the deformable meshes follow it)
  uint64_t device_refits = 0, device_tree_builds = 0;
  void* lbvh_scratch = nullptr;           // hk_rebuild_scene_trees
  size_t lbvh_scratch_cap = 0;
  // hk_load_scene (scene_load.hip): the mesh ranges the device is about to build (build_static_region neither threads nor folds them),
  // the size from which a deferred mesh is completed by the host instead, and what the last load did (hk_debug_last_load)
  std::vector<std::pair<uint32_t, uint32_t>> load_pending_ranges;
  uint32_t load_device_limit = HK_MESH_REBUILD_MAX_TRIANGLES;
  uint32_t last_load[4] = {0, 0, 0, 0};
  double last_load_ms[5] = {0, 0, 0, 0, 0};
  bool mesh_rebuild_one_workgroup = false;  // HK_DEBUG_OPT_MESH_REBUILD_ONE_WORKGROUP: the SAH build's top levels in one workgroup (A/B)
  const float4* d_prev_models = nullptr;  // 4 columns per instance, valid where DInstance::moved
  DevArray<uint32_t> d_noise;
  DevArray<uint32_t> d_tex_data;
  // textures from device memory (hk_update_textures_device, scene_layout.hip): the 256 thresholds of the sRGB encoding (host_logic.cpp
  // srgb_encode_thresholds; made at the first call), the producer's stream before the launch and the launch before the producer, which
  // textures' host copies (textures[i].texels) no longer hold what the device does, and what the last accepted call did
  float* tx_thresholds = nullptr;
  hipEvent_t tx_src_ready = nullptr, tx_src_read = nullptr;
  std::vector<uint8_t> tx_host_stale;
  uint32_t last_texture_update[3] = {0, 0, 0};  // hk_debug_last_texture_update: items, kernel launches, texels
  DScene scene{};

  // screen-space resources
  int W = 0, H = 0, RW = 0, RH = 0;
  int UW = 0, UH = 0;           // SMAA Tu4x output size, ceil(size * 2 / ratio) (post_process.rs:718-722)
  bool uv_fast = false;         // (k + 0.5) / size certified for div_by() on all four sizes (certify_uv_division)
  uint32_t mapped_parity = 0;   // frame parity whose planes the non-PREVIOUS ids of the double-buffered set name
  float ratio = 1.0f;
  void* buf[HK_BUF_COUNT] = {};
  size_t buf_bytes[HK_BUF_COUNT] = {};
  // private planes (no HkBuffer id): derived G-buffer planes and the denoiser's per-channel sets used
  // when all channels of a level run in one launch (the exposed internals hold the LAST channel, which
  // is what they hold after the reference's channel-by-channel loop)
  float* depth_plane = nullptr;       // position.w of the current frame's G-buffer (4-B taps)
  float* prev_depth_plane = nullptr;  // ... of the previous frame's (follows the frame parity like HK_BUF_PREVIOUS_POSITION)
  void* dn_g = nullptr;
  void* dn_extra[2][4] = {};
  float* dn_extra_var[2] = {};
  bool derived_dirty = false;
  // the host wrote HK_BUF_PREVIOUS_POSITION (hk_write_buffer) or holds its pointer (hk_device_ptr): prev_depth_plane is copied from its
  // .w again in front of the next anti-aliasing dispatch (a frame without such a write launches nothing)
  bool prev_depth_dirty = false;
  // scratch of the queue-based schedule of indirect_lit_ambient (hikari_hip.h HK_CTX_WAVEFRONT): ONE allocation, carved into
  // the planes of hkd::WfBuffers on first use and again after hk_resize
  void* wf_mem = nullptr;
  hkd::WfBuffers wf{};
  // wide trees of the trace stages (hk_kernels.hpp WideTrees): records derived ON THE DEVICE from ordering 0 of the trees the scene
  // blob holds, lazily - the mesh trees when the mesh-level region was rebuilt, the instance tree whenever it was uploaded, refit or
  // rebuilt (wide_*_dirty), in stream order right before the pass that walks them
  float4* wide_tlas = nullptr;
  float4* wide_blas = nullptr;
  uint32_t* wide_spill = nullptr;
  uint32_t* wide_tlas_rank = nullptr;   // [instance] / [primitive]: the position of its leaf in ordering 0 (the reference's tie rule)
  uint32_t* wide_blas_rank = nullptr;
  size_t wide_rank_instances = 0, wide_rank_primitives = 0;
  size_t wide_tlas_slots = 0, wide_blas_slots = 0, wide_spill_lanes = 0;
  bool wide_tlas_dirty = true, wide_blas_dirty = true;
  bool wide_mesh_check = true;                                  // the instance SET changed: a mesh no instance used before may have none yet
  std::vector<std::pair<uint32_t, uint32_t>> wide_meshes;       // (node_offset, node_count) of the mesh trees whose records exist, sorted
  int compute_units = 0;

  // uniforms
  HkFrame frame{};
  HkView view{};
  HkPreviousView pview{};
  HkLights lights{};
  bool have_frame = false;
  uint32_t taa = HK_TAA_JASMINE, upscale_kind = HK_UPSCALE_SMAA_TU4X;
  float upscale_sharpness = 0.0f;

  uint32_t band_index = 0, band_count = 1;
  std::vector<uint32_t> band_bounds;   // explicit split of the scaled render rows (hk_set_band_bounds): band_count + 1 entries, or empty = equal split
  uint32_t bounds_generation = 0;
  void* comm = nullptr;        // RCCL communicator state, owned by comm.cpp (hk_comm_init)
  uint32_t history_rows = HK_HISTORY_AUTO;  // exchange C rows asked for (hk_set_history_rows): a count, or derived per frame
  uint32_t history_now = 0;    // ... in force for the frame most recently begun (0 for a single band)
  hipEvent_t band_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // HK_FRAME_TIME_BAND: around stage TEMPORAL, around stage SPATIAL (main stream)
  bool band_timed = false;

  // ray queries (hk_cast_rays): pinned staging and device memory for one chunk of rays and their records, grown on demand
  uint8_t* query_staging = nullptr;
  uint8_t* query_device = nullptr;
  size_t query_capacity = 0;   // rays both hold

  // statistics
  unsigned long long* d_counters = nullptr;  // primary, tlas, blas, node steps, triangle tests, instance entries, closest hits (hk_light.hpp flush_counters)
  uint64_t frames = 0;
  uint32_t timing_mask = 0;
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> event_pool;
  double slot_ms[HK_TIMING_SLOTS] = {};
  uint64_t slot_launches[HK_TIMING_SLOTS] = {};
  hipEvent_t frame_start = nullptr, frame_stop = nullptr;
  bool frame_timed = false;
  float last_frame_ms = 0.0f;
};

namespace hk {
// ---- context.hip
int join_side(hk_ctx* c);   // the main stream waits for what was enqueued on the side stream (direct-light dispatches)
int join_post(hk_ctx* c);   // ... for the a-trous levels of the last frame (post_stream)
int join_all(hk_ctx* c);
// ---- scene_layout.hip
// wait for everything the context has enqueued, on ALL streams
int sync_all(hk_ctx* c);
// bring the device scene up to date with the host-side arrays (no-op when nothing is dirty)
int finalize_scene(hk_ctx* c);
// the instance-level region laid out from the mirrors into `blob` (finalize_scene; hk_change_scene_instances, which lets the device
// overwrite what the mirrors hold stale), and c->dyn_blob through pinned staging into the slot in use of a two-slot scene
int build_dynamic_region(hk_ctx* c, Blob& blob, DynOffsets& o, size_t mesh_bytes);
int upload_slot_staged(hk_ctx* c);
void update_shared_transform(hk_ctx* c);
void point_scene_at_slot(hk_ctx* c);
void repoint_scene(hk_ctx* c);   // ... where the slot or the allocation changed under a scene in use: the refit's own previous-model plane stays
size_t fold_leaf_navigators(std::vector<float4>& lo, std::vector<float4>& hi, size_t begin, size_t count);
void thread_orderings(const std::vector<HkNode>& src, const std::vector<std::pair<uint32_t, uint32_t>>& ranges, int orderings, std::vector<std::vector<HkNode>>& out);
// whether a scene of these mirror sizes keeps eight direction-threaded orderings (the estimate finalize_scene decides by)
bool wants_threaded(const hk_ctx* c, size_t n_nodes, size_t n_prims, size_t n_verts);
// the mesh-level region for these capacities: offsets of the sub-arrays (nodes, v0, v1, v2, vn, vuv) and its bytes
MeshRegion mesh_region_layout(const MeshSizes& caps, uint32_t orderings);
// ---- scene_load.hip
struct LoadMesh {
  uint32_t id;
  HkMeshIndex index;
  uint32_t n_tris;
};
// the trees of `meshes` built into their node ranges of every ordering, then read back into the builder and the mirror; `reference_if_unused`:
// a range no instance uses is left in reference form, as the host layout leaves it (hk_load_scene)
int build_on_device(hk_ctx* c, hk_scene_builder* b, const std::vector<LoadMesh>& meshes, uint32_t mode, uint32_t* launches, bool reference_if_unused);
// ---- scene_move.hip: a two-slot scene moved to a new allocation in stream order.  move_begin makes what the move needs and writes nothing
// of the context; the caller enqueues what fills the new allocation (move_planes lists it); move_commit switches the context over and
// retires what was replaced; until then move_abort leaves the scene the context had.
void retire(hk_ctx* c, void* p, hipEvent_t done);   // free `p` once `done` has passed (takes the event over)
void poll_retired(hk_ctx* c, bool wait);            // ... checked here, only behind a wait for the context's streams (hipFree may wait by itself); wait: free everything
MeshSizes move_room(const MeshSizes& need);         // the capacities a moved scene gets: half again the need, primitives and vertices in fours
struct SceneMove {
  MeshRegion mesh;               // of the new allocation `mem`, behind two instance-level slots of `dyn_capacity` bytes
  size_t dyn_capacity = 0;
  uint8_t *mem = nullptr, *extra = nullptr;   // extra: a device block of the caller's that lives as long as the move (hk_remove_meshes: its run table)
  float4* wide = nullptr;        // new wide records / ranks of the mesh trees, NULL where the move does not take them along
  uint32_t* rank = nullptr;
  hipEvent_t done[4] = {nullptr, nullptr, nullptr, nullptr};  // behind the move, one per allocation above (the last only with `extra`)
};
// one sub-array that moves: its list (0 nodes, 1 primitives, 2 vertices), its element size 1 << shift, its capacities in elements
struct MovePlane { const uint8_t* src; uint8_t* dst; uint32_t list, shift; size_t old_cap, new_cap; };
constexpr uint32_t HK_MOVE_PLANES = 8 + 3 + 2 + 2;   // (move_begin: `refusal` is the caller's text for a failed allocation; the ranks' 0xFF fill is enqueued there)
int move_begin(const hk_ctx* c, const MeshSizes& caps, size_t dyn_capacity, bool with_wide, bool with_rank, size_t extra_bytes, const char* refusal, SceneMove* m);
uint32_t move_planes(const hk_ctx* c, const SceneMove& m, MovePlane out[HK_MOVE_PLANES]);
void move_abort(const hk_ctx* c, SceneMove* m, bool enqueued);   // enqueued: work on c->stream may name the new allocations - it is waited for first
int move_commit(hk_ctx* c, SceneMove* m, int slot);        // `slot`: the instance-level slot in use from here on
int grow_instance_slots(hk_ctx* c, size_t dyn_capacity);   // (scene_append.hip) a two-slot scene moved, device to device in one launch, to an allocation whose instance-level slots hold `dyn_capacity` bytes each (hk_change_scene_instances)
// ---- scene_instances.hip: materials the builder holds beyond the context's - their texture ids checked, nothing written; taken into the mirror
int check_appended_materials(const hk_ctx* c, const hk_scene_builder* b);
int take_appended_materials(hk_ctx* c, const hk_scene_builder* b);
// ---- mesh_deform.hip, for hk_remove_meshes (scene_remove.hip): the records of the deformable meshes; then, `runs` being the surviving
// intervals per list (nodes, primitives, vertices), every record rebased and the meshes that lie in no run dropped - their device
// allocations go to `freed` for the caller to retire
void deform_mesh_records(const hk_ctx* c, std::vector<HkMeshIndex>& out);
void rebase_deform_meshes(hk_ctx* c, const std::vector<hk::CompactRun> runs[3], std::vector<void*>& freed);
const uint32_t* deformed_mesh_box(const hk_ctx* c, const HkMeshIndex& m);   // the box words of a mesh deformed on the device, or NULL
void deform_flushed(hk_ctx* c);                                              // every deformed mesh's box has reached the instance level by another way
// ---- scene_refit.hip
void free_refit(hk_ctx* c);
int begin_device_update(hk_ctx* c);
int prepare_refit(hk_ctx* c);
int reserve_refit(hk_ctx* c, size_t n_instances, size_t n_alias);   // the refit's side arrays for that many instances / alias entries (waits only where they grow)
int reserve_tree_scratch(hk_ctx* c, uint32_t n_instances, uint32_t n_emitters);
int build_trees_in_slot(hk_ctx* c, uint32_t mode);                 // both trees built over rf_inst_lo / rf_inst_hi and the emitters, in the slot in use (hk_rebuild_scene_trees' launches)
hkd::RefitScene refit_scene(hk_ctx* c);
// ---- mesh_deform.hip
void free_deform(hk_ctx* c);
int stage(hk_ctx* c, size_t bytes, uint8_t** out, int* k);   // a pinned staging buffer from the pool (c->df_stage[*k]: record its `done` event behind the reader)
// a caller's source in device memory (hk_deform_meshes_device, hk_update_textures_device): aligned, the context's device's or mapped host memory, `extent` bytes inside its allocation
int check_source(hk_ctx* c, uint32_t item, const char* what, const void* p, size_t align, size_t extent);
int repropagate_deformed(hk_ctx* c);   // after an instance refit: the deformed meshes' current boxes again (hk_refit_scene_instances)
int flush_deform(hk_ctx* c);           // the instance level of the meshes deformed since the last flush, once (frames, tree rebuilds, reads)
// motion vectors: motion_frame in front of a frame's first primary rays - which meshes are live, the instance table in stream
// order on the main stream, scene_epoch bumped where the live set changed (so that these primary rays are not pipelined past the table);
// motion_pass directly behind every launch_prepass, on its stream, over its rows - launches only while a mesh is live
int motion_frame(hk_ctx* c);
int motion_pass(hk_ctx* c, hipStream_t st, const hkd::DFrame& fr, const hkd::GBuffer& g, float jitter_x, float jitter_y, int y0, int y1);
}  // namespace hk
