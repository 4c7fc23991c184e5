// hk_kernels.hpp - kernel argument bundles and host launchers (implemented in kernels.hip)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hikari_hip.h"  // HkPresentTarget
#include "hk_device.hpp"

namespace hkd {

// group 1 of the reference pipelines (deferred_bindings.wgsl:3-12), row-major planes
struct GBuffer {
  float4* __restrict__ position;          // rgba32f: world xyz, clip depth
  uint32_t* __restrict__ normal;          // rgba8snorm
  float2* __restrict__ depth_gradient;    // rg32f
  float2* __restrict__ instance_material; // rg32f, id + 0.5
  float4* __restrict__ velocity_uv;       // rgba32f
  // derived planes (not part of the reference's bindings): written by k_prepass / k_derive_planes
  float* __restrict__ depth;              // position.w alone: 4-B taps for the spatial-reuse ray march
  float4* __restrict__ dn_g;              // (normalised stored normal xyz, instance id + 0.5): one 16-B tap for the denoiser
  // optional: k_prepass also evaluates full_screen_albedo (light.wgsl:1019-1042) for the pixels it covers and
  // writes it here (the frame path); null = the separate k_full_screen_albedo dispatch does it
  uint2* __restrict__ albedo_out;
  // the empty-tile plane of this frame's parity (one byte per 8x8 tile, tiles_x per row): k_prepass writes 1 where all the primary rays
  // of a tile missed (empty_out); the light kernels read it (empty_in) and skip the arithmetic whose result is then known.  Either is
  // null where the context cannot vouch for the plane (context.hip known_empty_plane)
  uint8_t* empty_out;
  const uint8_t* empty_in;
  // the kept-tile plane of the same parity (DESIGN 4 "Empty tiles"): the empty-tile byte (HK_TILE_EMPTY) plus HK_TILE_KEPT where the tile
  // was empty in the frame that last wrote these physical planes too - the byte k_prepass finds in empty_out before it overwrites it.
  // kept_out non-null says that the old byte may be trusted (context.hip kept_grant): the miss branch of a kept tile stores nothing,
  // every plane holds the background's constants already.  A light kernel whose own planes of this parity are in the same state is
  // handed this plane as its empty_in (otherwise the empty-tile plane, which never carries the bit) and skips its constant stores
  uint8_t* kept_out;
  // the OTHER parity's empty-tile plane, or null: the planes the post chain writes are not twinned by frame parity (the tone-mapped image
  // apart), so what they hold in a tile is what the frame before this one left there.  Where the context vouches for that frame's plane
  // and post chain (context.hip post_grant), the byte written to kept_out carries HK_TILE_POST_KEPT too if every ray of the tile missed
  // in that frame and in this one; demodulation and the a-trous levels are then handed the kept-tile plane and skip their constant stores
  const uint8_t* post_in;
  int tiles_x;
};
// Uniform-tile store elision.  The reference stores a packed reservoir to up to three buffers for EVERY pixel of EVERY light
// dispatch, background included (light.wgsl:1058-1069,1279-1287,1527-1532) - on a frame that is 64 % sky that is ~1 GB of HBM
// writes per frame that rewrite the same constant record over itself.  Per reservoir buffer and 8x8 tile the library keeps a
// small record: `id` = hash of the record ALL 64 slots of the tile hold, `src` = the id of the input tile that record was derived
// from (spatial_reuse's background branch re-packs its input), `valid` = serial number of the dispatch that wrote the tile
// uniformly (0: contents unknown / not uniform), `poison` = highest serial of a dispatch that stored into the tile from OUTSIDE
// (the reprojected scatter stores to previous_spatial).  A wave whose 64 pixels are all background may skip its tile store iff
// the tile already holds exactly that record: valid > poison && id == the record's id.  Contents of every buffer are therefore
// bit for bit what they are without the elision; only redundant traffic disappears.
struct TileMeta {
  unsigned long long id, src;
  uint32_t valid, poison, pad0, pad1;
};
// groups 5 + 6 for one light channel (light.wgsl:26-31,68-75; ping-pong light.rs:518-546)
struct LightTargets {
  const PackedReservoir* __restrict__ previous;  // binding 0
  PackedReservoir* current;                      // binding 1
  PackedReservoir* previous_spatial;             // binding 2
  PackedReservoir* spatial;                      // binding 3
  float* variance;                               // r32f
  uint2* render;                                 // rgba16f
  // HK_CTX_DETERMINISTIC_SCATTER (verification mode, nullptr otherwise): stores to previous_spatial are parked here
  // and applied by k_resolve_scatter - the store of the highest thread index wins, the oracle's resolution of the
  // reference's write-write race (light.wgsl:1063,1092-1095,1199-1202,1456-1459)
  int* det_winner;               // per previous_spatial slot: highest pixel index that stores to it (-1: none)
  int* det_to;                   // per pixel: the slot its parked store goes to (-1: none)
  PackedReservoir* det_pending;  // per pixel: the parked value
  // Round 6, single contexts: the LIGHT form of the same rule (hk_light.hpp store_previous_spatial, kernels.hip k_resolve_scatter_lite).
  // A store to the pixel's OWN slot goes straight to previous_spatial - one pixel owns a slot, such stores do not race with each other -
  // and only a store to ANOTHER pixel's slot is parked and competes in det_winner.  The resolve pass applies the highest such store
  // unless the slot's owner stored to it too and has the higher index: the same winner as the full rule, without 68 B per pixel of
  // parked traffic, with the uniform-tile store elision and the frame pipelining left on.
  int det_lite;
  // uniform-tile store elision (TileMeta above); all null when it is off (verification mode, band-sharded or row-unaligned dispatches)
  TileMeta* m_current;
  TileMeta* m_spatial;
  TileMeta* m_previous_spatial;
  uint32_t serial;  // of this dispatch, > 0, increasing
  int tiles_x;      // 8x8 tiles per row of the render image
  int rw;           // render width (reservoir index = x + rw * y)
  int slots;        // rw * rh: entries the passes index of every reservoir buffer, and of every parked-store plane (hk_light.hpp previous_slot lets no store land beyond)
};
// The background's known records (kernels.hip k_spatial_known_fill / k_spatial_reuse; DESIGN 4 "Empty tiles").  spatial_reuse's
// background branch stores pack(unpack(its input)); of the two records the temporal passes store to a background pixel - entry 0:
// pack(zero_reservoir()), k_indirect's; entry 1: the pack of set_reservoir(zero, zero_sample, 0), k_direct_lit's - that re-pack is a
// constant, computed once per context by a one-wave kernel with the very functions the long way uses.  A wave whose input tile record
// names one of the two input ids stores `output` and marks its tile with `output_id`: no load, no unpack, no pack, no hash.
// Read-only to every kernel but the one that fills it.
struct SpatialKnownEntry {
  PackedReservoir output;
  unsigned long long input_id, output_id;
};
struct SpatialKnown {
  SpatialKnownEntry e[2];
};
// The queue-based schedule of indirect_lit_ambient (kernels_wavefront.hip): what a path carries from stage to stage, in
// planes indexed by path slot, plus the ray queues and their counters.  `cap` = the most paths one dispatch can have
// (the pixels of the render image).
struct WfBuffers {
  uint32_t* ctr;       // 192 counters, zeroed per dispatch: [s] paths alive at bounce s, [64 + s] shadow rays / [128 + s] claimed rays of trace stage s
  uint32_t* pixel;     // [slot] x + rw * y
  float4* state;       // 9 planes of `cap`: random | position, pdf | normal, pending | transport | radiance | first hit position | first hit normal | radiance to add if the shadow ray is clear | if it is occluded
  float4 *cr0, *cr1;   // closest-hit ray of the bounce: (origin, -), (direction, pdf of the direction)
  float4 *sr0, *sr1;   // shadow ray of the bounce: (origin, max_distance), (direction, early-out distance)
  uint32_t* sr2;       // ... and the instance its walk excludes (the sampled emitter)
  float4* ch0;         // closest hit: (distance, u, v, primitive index bits)
  uint32_t* ch1;       // ... its instance index (U32_MAX: miss)
  uint32_t* sh;        // instance the shadow ray hit (U32_MAX: clear)
  uint32_t* alive[2];  // slots alive at a bounce (= the closest-hit rays of that bounce's trace stage), ping-pong
  uint32_t* shadow[2]; // slots whose shadow ray the trace stage walks, ping-pong
  uint32_t cap;
  // HK_WF_TIMELINE=1 (tools/wf_timeline.py; null otherwise, and then the instrumented instantiation of k_wf_trace never runs): 32
  // u64 per trace stage, zeroed per dispatch - [0] ~first wave start, [1] ~first time a wave found the queue exhausted, [2] last
  // wave exit (wall_clock64 ticks; ~x = UINT64_MAX - x so that atomicMax keeps the minimum), [3] sum of the waves' resident ticks,
  // [4] waves, [5] most node steps of one ray, [6] node steps, [7] rays, [8..23] rays by floor(log2(node steps + 1))
  // HK_CTX_COUNT_WALKS (round 5): the COUNTING twin of k_wf_trace_wide writes [0..4] as above and [8] records fetched, [9] of them in
  // the instance tree, [10] triangle tests, [11] instance entries, [12] rays claimed, [13] of them any-hit, [14] closest hits found,
  // [15] pieces of walks handed to idle lanes
  unsigned long long* timeline;
  uint32_t timeline_mode;  // 0: none (the product), 1: the timeline twin, 2: the counting twin
};
// Wide trees for the queue-based trace stage and the primary rays of scenes in global memory (round 4; kernels_wavefront.hip
// k_build_wide / k_wf_trace_wide, kernels.hip k_prepass<*, 4>, hk_wide.hpp; DESIGN 4 "Wide walk").
// One 128-B record per INNER node of a flatten_custom tree, at the node's own position in a parallel array: the boxes and links
// of its (up to four) grandchildren - four 32-B box-nodes, lo = (min.xyz, link), hi = (max.xyz, -).  link: HK_LEAF | id = a leaf
// (triangle of the mesh / instance), < HK_LEAF = position of an inner node (its record), 0xFFFFFFFF = no child.  The record of a
// tree's root (which flatten_custom does not store) sits in the tree's LAST slot (always a leaf's).  ONE ordering: the walk keeps
// a per-lane stack and takes the children nearest first, so the eight direction-threaded copies are not needed here.
// Ranks (round 5): the position of every leaf in the REFERENCE's own flattening (ordering 0) - the order in which the reference's
// stackless walk meets the leaves.  Of two candidates at exactly the same distance the reference keeps the one it meets first
// (light.wgsl:415-424: `<`), i.e. the one of smaller rank - instance leaves first, then triangle leaves inside the instance; the
// wide walk, which meets them nearest-box first, decides the tie by the ranks and so returns the reference's hit, bit for bit.
struct WideTrees {
  const float4* tlas;   // records of the instance tree: 8 float4 per slot, tlas_count slots
  const float4* blas;   // records of every mesh tree: slot node_offset + local position
  const uint32_t* tlas_rank;  // [instance] position of its leaf in the instance tree (ordering 0)
  const uint32_t* blas_rank;  // [primitive] position of its leaf in its mesh tree (ordering 0)
  uint32_t tlas_count;  // (its root: slot tlas_count - 1)
  unsigned long long* lost;  // counts stack entries that fit neither part (HkStats::wide_stack_lost)
  uint32_t* spill;      // stack entries beyond the LDS part: HK_WIDE_SPILL u32 per lane of the persistent launch (the trace stage;
                        // nullptr where only the prepass - whose lanes keep the rest in private memory - walks them)
};
// Instance motion on the device (kernels_scene.hip): the arrays of the instance-level region the refit kernels rewrite, plus
// the refit's own side arrays.
struct RefitUpdate {       // one record per instance whose transform changed (read from pinned host memory)
  uint32_t instance;
  uint32_t moved;          // 0: the instance moved in the previous update but not in this one (its `moved` flag is cleared)
  float model[16];         // new model matrix, column-major
  float aabb_center[3], aabb_half[3];  // the mesh's local box (bevy Aabb), instance.rs:286-296
};
struct MaterialUpdate {    // one record per material whose values changed (hk_update_materials; read from pinned host memory)
  uint32_t material;
  uint32_t pad[3];
  float4 rows[4];          // the material's four float4 of the device layout (scene_layout.hip build_dynamic_region)
};
// Mesh deformation (kernels_deform.hip, kernels_tree.hip; host side mesh_deform.hip): one mesh BLAS of n triangles as the binary tree
// behind its flat layout - internal nodes in the preorder of ordering 0 (root 0), leaves in ordering 0's order as tree nodes n - 1 + j -
// with the work planes of a bottom-up refit.
struct MeshTree {
  uint32_t n;
  uint32_t *parent, *left, *right, *first, *last;  // per internal node (left = the child ordering 0 puts first)
  uint32_t *leaf_parent, *leaf_shape;              // per leaf: its parent, its triangle (local index)
  uint32_t* arrived;                               // per internal node: bottom-up visit counter (zeroed before every refit)
  uint8_t* swap;                                   // per internal node: bit o set = the second child comes first in ordering o
  float4 *node_lo, *node_hi;                       // per tree node (2n - 1)
  float4 *tri_lo, *tri_hi;                         // per triangle: its box
};
// One item of a batched deformation (hk_deform_meshes; kernels_deform.hip k_deform_*, kernels_tree.hip k_deform_boxes / k_deform_emit):
// everything the kernels need of the item's mesh.  The table lies in the pinned staging block of the call, with the host data of the
// items behind it, and is read from there (as RefitUpdate records are).
struct DeformItem {
  uint32_t kind;                     // HK_DEFORM_VERTICES / HK_DEFORM_SKIN / HK_DEFORM_MORPH / HK_DEFORM_MORPH_SKIN
  uint32_t n_vertices, n_tris, n_joints;
  const float *positions, *normals;  // VERTICES: staged, 3 floats per vertex (normals: or NULL = keep)
  const float4* palette;             // SKIN, MORPH_SKIN: the staged joint matrices, copied to joint_mats by k_deform_begin
  float4* joint_mats;
  const float4 *bind_pos, *bind_nrm, *weights;
  const uint2* joints;
  float4 *pos, *vn;                  // the mesh's position scratch plane; its normals in the normal plane
  uint32_t* box;                     // the mesh box, 6 order-preserving words
  float4 *v0, *v1, *v2;              // the mesh's first triangle in the triangle planes
  MeshTree tree;
  float4* nodes;                     // the mesh's first node (lo) in ordering 0 of the mesh-level node array
  uint32_t pos_stride, nrm_stride;   // VERTICES: floats from one vertex to the next in positions / normals (3: packed staging; hk_deform_meshes_device: the caller's)
  // HK_DEFORM_RECOMPUTE_NORMALS (hk_deform_meshes_device; NULL otherwise): the mesh's face-vector plane, one per triangle, and its corner
  // list - corner_tri[corner_off[v] .. corner_off[v + 1]) are the triangles that name vertex v, ascending, one entry per naming corner
  float4* face;
  const uint32_t *corner_off, *corner_tri;
  // HK_DEFORM_MORPH / HK_DEFORM_MORPH_SKIN (hikari_hip.h hk_set_mesh_morph_targets): the mesh's morph set - packed planes of 3 floats per
  // vertex, the deltas target-major (delta k of vertex v at [(k * n_vertices + v) * 3]; morph_dn NULL: the normals do not morph) - the
  // item's weights as given (staged, or the caller's device memory), and what k_deform_begin makes of them in the mesh's own memory: a
  // copy of the n_targets weights and the ascending list of the active targets, its length in morph_active[n_targets]
  const float *morph_base_p, *morph_base_n, *morph_dp, *morph_dn;
  const float* morph_src;
  float* morph_w;
  uint32_t* morph_active;
  uint32_t n_targets, pad_;
};
// A workgroup of a segmented launch: 256 consecutive elements of ONE segment (item, tree), from `first` on.  The host writes one entry
// per workgroup, so no workgroup - and no wave - spans two segments, whatever their sizes and however many there are.
struct SegmentBlock {
  uint32_t segment, first;
};
// One item of hk_update_textures_device (kernels_scene.hip k_update_textures): a rectangle of one texture and the caller's strided source
// for it.  The table lies in the pinned staging block of the call; a workgroup (SegmentBlock: segment = item, first = a row of the
// rectangle) converts `rows` rows from `first` on.
struct TextureItem {
  const uint8_t* src;                // DEVICE memory: element (x, y, ch) at src + y * stride_y + x * stride_x + ch * stride_c
  uint64_t stride_x, stride_y, stride_c;
  uint32_t dst;                      // the texel of the rectangle's corner (x0, y0), counted from the start of the texel buffer
  uint32_t pitch;                    // the texture's width
  uint32_t width, height;            // the rectangle
  uint32_t format, channels;         // HK_TEXELS_*; 1, 3 or 4
  uint32_t mode;                     // HK_TEXTURE_ITEM_*
  uint32_t rows;                     // rows of the rectangle per workgroup
  uint32_t index;                    // the texture: its descriptor becomes `info`
  uint32_t pad[3];
  uint4 info;
};
constexpr uint32_t HK_TEXTURE_ITEM_ENCODE = 1u;   // rgb are linear light of an sRGB texture: encoded through the thresholds
constexpr uint32_t HK_TEXTURE_ITEM_PACKED = 2u;   // four channels side by side, every element aligned to all four: one 4 / 8 / 16 B load
// One source of hk_add_meshes_device (kernels_scene.hip k_assemble_meshes): a declared mesh's arrays in the caller's DEVICE memory and where
// its reference records go in the call's device block.  The table lies in the pinned staging block of the call; a workgroup
// (SegmentBlock: segment = source, first = a triangle, or a vertex for the workgroups behind the triangles') takes 256 of them.
struct MeshSourceItem {
  const uint8_t *positions, *normals;  // 3 floats per vertex at + v * stride
  const uint8_t* uvs;                  // 2 floats per vertex, or NULL: (0, 0)
  const uint32_t* indices;             // or NULL: the identity list
  uint4* prims;                        // HkPrimitive records: 3 x 16 B per triangle {position, index}
  uint4* verts;                        // HkVertex records: 2 x 16 B per vertex {position, u} {normal, v}
  uint32_t n_vertices, n_tris;
  uint32_t stride_p, stride_n, stride_uv;
  uint32_t strip;                      // 1: triangle t names (t, t + 1, t + 2) of the list, the first two swapped for odd t
  uint32_t pad[2];
};
static_assert(sizeof(MeshSourceItem) == 80, "the item table is laid out by the host");
// One instance of a deformed mesh (kernels_scene.hip k_mesh_instances): the mesh's box words, and the emitter record to write if it emits
struct MeshInstanceEntry {
  uint32_t instance;
  uint32_t record;                   // index into the launch's RefitUpdate records, HK_U32_MAX: no emitter
  const uint32_t* box;
};
// hk_change_scene_instances (kernels_scene.hip k_carry_instances / k_derive_instances): one record per instance of the NEW instance
// level, in pinned memory
struct InstanceDerive {
  uint32_t origin;                   // the id the instance had in the old level, HK_U32_MAX: it is new
  uint32_t emitter;                  // its emitter in the new level (and its RefitUpdate record), HK_U32_MAX: none
  const uint32_t* box;               // the box words of its mesh where the mesh was deformed on the device, else NULL: the builder's box
  float aabb_center[3], aabb_half[3];
  uint32_t pad[2];
};
static_assert(sizeof(InstanceDerive) == 48, "three 16-B loads per record");
// One tree of a segmented derivation of wide records (kernels_wavefront.hip k_build_wide_trees): offsets into the launch's arrays
struct WideTreeSegment {
  uint32_t node_offset, count;       // its slots in the node array (ordering 0)
  uint32_t wide_offset;              // its first record (in records of 8 float4)
  uint32_t rank_offset;              // where its leaf ids start in the rank array
};
// One mesh of a forest build (kernels_tree.hip launch_forest_build; hk_load_scene): the trees of many meshes built together
struct ForestMesh {
  uint32_t tri_begin, n_tris;   // the mesh's positions in the batch: the meshes of a batch tile [0, all its triangles)
  uint32_t primitive;           // its first triangle in the triangle planes
  uint32_t node_offset;         // its first node in the mesh-level node array
};
struct RefitScene {
  DInstance* instances;
  float4* prev_models;                   // 4 columns per instance
  float4 *inst_lo, *inst_hi;             // world AABB per instance
  const uint32_t* emissive_of_instance;  // emitter index or U32_MAX
  DEmissive* emissives;
  float2* alias;
  float* alias_scratch;                  // 5 floats per alias entry
  const float4* materials;
  const float4 *tri_v0, *tri_v1, *tri_v2;
};
// groups 3 + 4 of the denoise pipeline (denoise.wgsl:10-28), for up to three channels per launch
struct DemodTargets {
  const uint2* __restrict__ albedo;     // rgba16f, full size
  const float* variance[3];             // light variance per channel
  const uint2* render[3];               // light render per channel
  uint2* output[3];                     // internal_texture_0 per channel
  float* internal_variance[3];
  const uint8_t* empty_tiles;           // the frame's empty-tile plane (GBuffer), or null - or its kept-tile plane (context.hip post_grant)
  int tiles_x;
};
struct DenoiseTargets {
  const uint2* __restrict__ albedo;
  const float4* __restrict__ dn_g;              // (normalize(unpack4x8snorm(normal)), instance id + 0.5) per full-size pixel
  const float* __restrict__ depth;              // position.w per full-size pixel
  const float2* __restrict__ depth_gradient;
  const uint2* input[3];                        // internal_texture_<level> per channel
  uint2* output[3];                             // internal_texture_<level+1> / denoise_render[channel]
  const float* internal_variance[3];
  // optional, level 3 with all channels in the launch: also apply tone_mapping.wgsl:21-32 to the sum of the
  // (f16-rounded) channel outputs and write tone_mapping_output (the frame path); null = separate dispatch
  uint2* tone_mapped;
  float clear_color[4];
  const uint8_t* empty_tiles;                   // the frame's empty-tile plane (GBuffer), or null - or its kept-tile plane (context.hip post_grant)
  int tiles_x;
  // the tone-mapped image IS twinned by frame parity: its store may be skipped only in a tile that carries HK_TILE_KEPT as well as
  // HK_TILE_POST_KEPT, and only if the last frame of this parity wrote this clear colour there (context.hip post_grant); 0 = always store
  int tone_kept;
};

// what an a-trous tap needs of a G-buffer pixel besides its depth: the normal exactly as the filter derives it
// from the rgba8snorm texel (denoise.wgsl:226,262: normalize(textureLoad(normal_texture).xyz)) and the instance id
__device__ __forceinline__ float4 denoise_geometry(uint32_t packed_normal, float instance) {
  const f3 n = normalize(xyz(unpack4x8snorm(packed_normal)));
  return make_float4(n.x, n.y, n.z, instance);
}

struct Pixel { int x, y; bool valid; };

// ---- uniform-tile store elision helpers: every call is made by ALL live lanes of a wave with wave-uniform arguments
__device__ __forceinline__ unsigned long long record_id(const PackedReservoir& p) {
  const uint32_t w[16] = {p.radiance.x, p.radiance.y, p.random.x, p.random.y, f2u(p.visible_position.x), f2u(p.visible_position.y), f2u(p.visible_position.z),
                          f2u(p.visible_position.w), f2u(p.sample_position.x), f2u(p.sample_position.y), f2u(p.sample_position.z), f2u(p.sample_position.w),
                          p.visible_normal, p.sample_normal, p.reservoir.x, p.reservoir.y};
  unsigned long long h = 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    h ^= (unsigned long long)w[k] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  return h | 1ull;
}
__device__ __forceinline__ bool wave_leader() { return (int)__lane_id() == __ffsll((long long)__ballot(1)) - 1; }
// the 8x8 tile this wave covers (wave-uniform by construction of pixel_of_thread, valid lane or not)
__device__ __forceinline__ int wave_tile(const Pixel& px, int tiles_x) {
  const int lane = threadIdx.x & 63;
  return ((px.y - (lane >> 3)) >> 3) * tiles_x + ((px.x - (lane & 7)) >> 3);
}
// the empty-tile plane: is the 8x8 tile of this wave (pixel_of_thread; called by its valid lanes only - their tile lies in the image) one
// whose primary rays all missed this frame?  Wave-uniform, and known to be: the byte is read through the first lane.
// The byte itself: 0 = not known to be empty (or no plane), HK_TILE_EMPTY = empty; in the kept-tile plane also HK_TILE_KEPT = empty in the
// last frame of this parity too (the parity's twinned planes hold the background's constants) and HK_TILE_POST_KEPT = empty in the frame
// before this one too (the post chain's planes, which every frame writes, hold theirs) - GBuffer.  Neither is ever set without HK_TILE_EMPTY.
#define HK_TILE_EMPTY 1
#define HK_TILE_KEPT 2
#define HK_TILE_POST_KEPT 4
__device__ __forceinline__ int wave_tile_state(const uint8_t* __restrict__ plane, const Pixel& px, int tiles_x) {
  if (!plane) return 0;
  const int tile = __builtin_amdgcn_readfirstlane(wave_tile(px, tiles_x));
  return __builtin_amdgcn_readfirstlane((int)plane[tile]);
}
__device__ __forceinline__ bool wave_tile_known_empty(const uint8_t* __restrict__ plane, const Pixel& px, int tiles_x) { return wave_tile_state(plane, px, tiles_x) != 0; }
// ... and for the row-shaped waves of the stencil kernels (pixel_of_thread_rows): do this pixel and its neighbours up to `reach` pixels
// away that lie in the image (reach <= 8: the four corners of the window name every tile it touches) all lie in empty tiles?  Per lane
// (a wave is one row of 64 pixels there: y and with it the two tile rows are wave-uniform and kept in scalar registers)
// The byte itself: the AND of the bytes of every tile within reach (every non-zero byte carries HK_TILE_EMPTY: 0 = some tile is not known
// to be empty; HK_TILE_KEPT / HK_TILE_POST_KEPT survive only where every tile within reach has them)
__device__ __forceinline__ int pixel_tile_bits(const uint8_t* __restrict__ plane, int tiles_x, int x, int y, int reach, int width, int height) {
  const int yu = __builtin_amdgcn_readfirstlane(y);
  const uint8_t* __restrict__ row0 = plane + (max(yu - reach, 0) >> 3) * tiles_x;
  const uint8_t* __restrict__ row1 = plane + (min(yu + reach, height - 1) >> 3) * tiles_x;
  if (reach == 0) return row0[(uint32_t)x >> 3];
  const uint32_t x0 = (uint32_t)max(x - reach, 0) >> 3, x1 = (uint32_t)min(x + reach, width - 1) >> 3;  // (unsigned: 32-bit offsets from the scalar row address)
  return row0[x0] & row0[x1] & row1[x0] & row1[x1];
}
__device__ __forceinline__ bool pixel_known_empty(const uint8_t* __restrict__ plane, int tiles_x, int x, int y, int reach, int width, int height) {
  return pixel_tile_bits(plane, tiles_x, x, y, reach, width, height) != 0;
}
__device__ __forceinline__ bool tile_holds(const TileMeta* m, int tile, unsigned long long id) {
  const TileMeta v = m[tile];
  return v.valid > v.poison && v.id == id;
}
__device__ __forceinline__ void tile_mark(TileMeta* m, int tile, unsigned long long id, unsigned long long src, uint32_t serial) {
  if (wave_leader()) {
    m[tile].id = id;
    m[tile].src = src;
    m[tile].valid = serial;
  }
}
__device__ __forceinline__ void tile_unknown(TileMeta* m, int tile) {
  if (wave_leader()) m[tile].valid = 0u;
}

// A wave's 64 reservoir records, written as full cache lines.  A lane holds its pixel's 64-B record in four 16-B
// chunks; storing them directly makes every store instruction touch 64 different lines, 16 B each, and the L2 has to
// stitch the lines together (nontemporal stores, which skip that, run these kernels 2x slower).  Here the wave
// transposes through LDS: instruction k writes chunks 64k..64k+63 of the tile in memory order, i.e. two rows of
// eight pixels = 2 x 512 contiguous bytes.  ALL lanes of the wave must call it (wave-uniform control flow);
// `write` says whether this lane's record is to be stored.  lds: 4 x 65 uint4 per wave (padded against bank conflicts).
constexpr int HK_TILE_LDS_UINT4 = 4 * 65;
__device__ __forceinline__ void store_packed_tile(uint4* lds, PackedReservoir* __restrict__ buf, int width, const Pixel& px, const PackedReservoir& p, bool write) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wmask = __ballot(write);
  if (wmask == 0ull) return;
  lds[0 * 65 + lane] = make_uint4(p.radiance.x, p.radiance.y, p.random.x, p.random.y);
  lds[1 * 65 + lane] = make_uint4(f2u(p.visible_position.x), f2u(p.visible_position.y), f2u(p.visible_position.z), f2u(p.visible_position.w));
  lds[2 * 65 + lane] = make_uint4(f2u(p.sample_position.x), f2u(p.sample_position.y), f2u(p.sample_position.z), f2u(p.sample_position.w));
  lds[3 * 65 + lane] = make_uint4(p.visible_normal, p.sample_normal, p.reservoir.x, p.reservoir.y);
  __builtin_amdgcn_wave_barrier();  // LDS operations of one wave execute in order; this only pins the compiler's schedule
  // tile origin: this lane's pixel minus its position in the 8x8 tile (valid or not, the arithmetic is the same)
  const int tile_x0 = px.x - (lane & 7), tile_y0 = px.y - (lane >> 3);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int m = k * 64 + lane, record = m >> 2, part = m & 3;
    const uint4 v = lds[part * 65 + record];
    if ((wmask >> record) & 1ull) {
      const int x = tile_x0 + (record & 7), y = tile_y0 + (record >> 3);
      reinterpret_cast<uint4*>(buf + (x + width * y))[part] = v;
    }
  }
  __builtin_amdgcn_wave_barrier();  // the next call reuses the buffer
}

// XCD_BANDS = true: linear workgroup ids are remapped so that each XCD (dispatcher: block b -> XCD b % 8) works on one
// contiguous eighth of the image and gather passes find their neighbours' data in that XCD's L2.  false: tiles go
// round-robin over the XCDs - for the ray kernels, whose cost per tile varies a lot and which gather nothing from
// neighbouring pixels, balance across the XCDs is worth more than locality.
template <bool XCD_BANDS = true>
__device__ __forceinline__ Pixel pixel_of_thread(int width, int row_begin, int row_end) {
  const int tiles_x = (width + 15) >> 4;
  const uint32_t nb = gridDim.x;
  uint32_t b = blockIdx.x;
  const uint32_t per = nb >> 3;
  // (a launch of a few workgroups per CU - one band of a multi-GPU split - has nothing to balance: keep the bands)
  if ((XCD_BANDS || nb < 2048u) && per > 0 && b < per * 8u) b = (b & 7u) * per + (b >> 3);
  const int tile_x = (int)(b % (uint32_t)tiles_x), tile_y = (int)(b / (uint32_t)tiles_x);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  Pixel p;
  p.x = tile_x * 16 + (wave & 1) * 8 + (lane & 7);
  p.y = row_begin + tile_y * 16 + (wave >> 1) * 8 + (lane >> 3);
  p.valid = p.x < width && p.y < row_end;
  return p;
}

// The streaming / stencil kernels' mapping (demodulation, a-trous): a wave covers W x (64 / W) pixels and a workgroup four such
// strips stacked, so that a wave's load of a 4-byte plane is whole 128-B lines instead of eight 32-B pieces of eight lines (the
// 8 x 8 tiles above suit gathers and rays).  XCD_BANDS as above.  Measured (Cornell 1080p, round 2): demodulation 0.071 ms with
// 8 x 8 tiles -> 0.047 (32 x 2) -> 0.040 (64 x 1, bands); the a-trous levels 0.072 -> 0.064 by going round-robin, any shape.
template <int W, bool XCD_BANDS>
__device__ __forceinline__ Pixel pixel_of_thread_rows(int width, int row_begin, int row_end) {
  constexpr int H = 64 / W;  // of a wave
  const int tiles_x = (width + W - 1) / W;
  uint32_t b = blockIdx.x;
  const uint32_t nb = gridDim.x, per = nb >> 3;
  if (XCD_BANDS && per > 0 && b < per * 8u) b = (b & 7u) * per + (b >> 3);
  const int tile_x = (int)(b % (uint32_t)tiles_x), tile_y = (int)(b / (uint32_t)tiles_x);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  Pixel p;
  p.x = tile_x * W + (lane & (W - 1));
  p.y = row_begin + tile_y * (4 * H) + wave * H + (lane / W);
  p.valid = p.x < width && p.y < row_end;
  return p;
}

// Motion vectors of deforming meshes (kernels_motion.hip k_motion_velocity; host side mesh_deform.hip): per instance the plane of its mesh's
// PREVIOUS local positions (one float4 per vertex, keyed by vertex id) and the vertices it holds, or NULL - the mesh has no motion this frame
struct MotionEntry {
  const float4* previous;
  uint32_t n_vertices, pad;
};
static_assert(sizeof(MotionEntry) == 16, "one 16-B load per look-up; staged and copied in 16-B units");
struct MotionTable {
  const MotionEntry* entries;
  uint32_t n_instances;
  unsigned int* rewritten;   // pixels rewritten (hk_debug_last_motion), or NULL: not counted
};

}  // namespace hkd

#define HK_LDS_SCENE_BYTES 32768u  // scenes up to this size are copied into LDS by the ray kernels (lds_bytes_for)

namespace hk {
static inline dim3 grid_for_rows(int wave_width, int width, int rows) {  // pixel_of_thread_rows<wave_width, *>
  int wg_rows = 4 * (64 / wave_width);
  int tiles_x = (width + wave_width - 1) / wave_width, tiles_y = (rows + wg_rows - 1) / wg_rows;
  return dim3((unsigned)(tiles_x * tiles_y), 1, 1);
}
static inline dim3 grid_for(int width, int rows) {
  int tiles_x = (width + 15) / 16, tiles_y = (rows + 15) / 16;
  return dim3((unsigned)(tiles_x * tiles_y), 1, 1);
}

void launch_prepass(hipStream_t st, const hkd::DScene& sc, const hkd::DFrame& fr, const float* inverse_view_proj, const float* view_proj,
                    const float* prev_view_proj, const float4* prev_models, float jitter_x, float jitter_y, const hkd::GBuffer& g, int y0, int y1,
                    unsigned long long* counters, const hkd::WideTrees* wide = nullptr);
// directly behind launch_prepass, same stream, same rows, while a mesh has live previous positions (kernels_motion.hip)
void launch_motion_velocity(hipStream_t st, const hkd::DScene& sc, const hkd::DFrame& fr, const float* inverse_view_proj, const float* view_proj,
                            const float* prev_view_proj, const float4* prev_models, float jitter_x, float jitter_y, const hkd::GBuffer& g, const hkd::MotionTable& mt,
                            int y0, int y1);
void launch_mesh_previous_fill(hipStream_t st, const float4* v0, const float4* v1, const float4* v2, uint32_t n_tris, float4* pos, uint32_t n_vertices);
void launch_albedo(hipStream_t st, const hkd::DScene& sc, const hkd::DFrame& fr, const hkd::GBuffer& g, void* albedo, int y0, int y1);
void launch_direct(hipStream_t st, bool emissive_lit, const hkd::DScene& sc, const hkd::DFrame& fr, const hkd::GBuffer& g, const hkd::LightTargets& t,
                   int y0, int y1, unsigned long long* counters);
void launch_indirect(hipStream_t st, bool multiple_bounces, const hkd::DScene& sc, const hkd::DFrame& fr, const hkd::GBuffer& g,
                     const hkd::LightTargets& t, int y0, int y1, unsigned long long* counters, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// the same dispatch as launch_indirect(multiple_bounces = true), scheduled through ray queues (kernels_wavefront.hip)
// wide: records of the trees for the trace stages (nullptr members = the threaded walk)
void launch_build_wide(hipStream_t st, const float4* nodes, uint32_t count, float4* wide, uint32_t* rank);  // one flatten_custom tree (ordering 0) -> its records; rank[leaf id] = the leaf's position
// ... of many trees in ONE launch: tree k = trees[k] (pinned), its slots from nodes + 2 node_offset, records from wide + 8 wide_offset, ranks from rank + rank_offset
void launch_build_wide_trees(hipStream_t st, const hkd::WideTreeSegment* trees, const hkd::SegmentBlock* blocks, uint32_t n_blocks, const float4* nodes, float4* wide,
                             uint32_t* rank);
// what WideTrees::spill must hold: wide_trace_lanes(compute_units) x wide_spill_entries() u32 (the lanes of the persistent trace launch
// x the stack entries a lane keeps beyond LDS) - asked of the file that launches the kernel, so that the two cannot disagree
size_t wide_trace_lanes(int compute_units);
size_t wide_spill_entries();
// trace_events: nullptr, or 2 x (bounces + 1) events - start / stop of every trace launch (HK_TIMING_TRACE_STAGES)
void launch_indirect_wavefront(hipStream_t st, const hkd::DScene& sc, const hkd::DFrame& fr, const hkd::GBuffer& g, const hkd::LightTargets& t,
                               const hkd::WfBuffers& w, int y0, int y1, int compute_units, hipEvent_t start = nullptr, hipEvent_t stop = nullptr,
                               const hkd::WideTrees* wide = nullptr, hipEvent_t* trace_events = nullptr);
void launch_copy_region(hipStream_t st, void* dst, const void* src, size_t bytes);
// hk_add_meshes: up to HK_COPY_SEGMENTS copies in ONE launch - the sub-arrays of a scene moved to a roomier allocation, the staged node
// ranges of every ordering; dst / src 16-B aligned, `bytes` whole 4-B words
#define HK_COPY_SEGMENTS 16u
struct CopySegments {
  struct Segment { uint4* dst; const uint4* src; size_t bytes; } seg[HK_COPY_SEGMENTS];
  uint32_t count = 0;
  bool overflow = false;  // add() was asked for more than the table holds: the caller must not launch
  void add(void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    if (count >= HK_COPY_SEGMENTS) { overflow = true; return; }
    seg[count].dst = (uint4*)dst; seg[count].src = (const uint4*)src; seg[count].bytes = bytes;
    ++count;
  }
};
void launch_copy_segments(hipStream_t st, const CopySegments& segments);
// hk_remove_meshes (scene_remove.hip): the surviving runs of many planes moved to a new allocation in ONE launch.  Three run lists - the
// surviving intervals in node, primitive and vertex units, `dst` their prefix sum - and up to HK_COMPACT_PLANES planes, each with its old
// base, its new base, the list it follows and its element size 1 << shift (4, 8, 16, 32 or 128 B); the tables lie in device memory.  A
// work item is HK_COMPACT_PIECE bytes of a plane's DESTINATION: the load is the same for one run of a gigabyte and for three thousand
// runs of a kilobyte.  Bases are 16-B aligned; a run's source is not, in the 4-B and 8-B planes.
#define HK_COMPACT_PLANES 16u
#define HK_COMPACT_PIECE 16384u
struct CompactRun { uint32_t src, dst, count, pad; };
struct CompactPlane { const uint8_t* src; uint8_t* dst; uint32_t list, shift; uint64_t first_piece; };
struct CompactArgs {
  const CompactPlane* planes;
  const CompactRun* runs[3];
  uint32_t n_planes, n_runs[3], total[3];   // total: the surviving elements of a list
  uint64_t n_pieces;
};
// where element `x` of a list lies once only the runs are left: x minus the removed elements in front of it (host and device)
__host__ __device__ inline uint32_t compact_rebase(const CompactRun* runs, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;   // the first run that begins behind x
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (runs[mid].src <= x) lo = mid + 1; else hi = mid;
  }
  if (!lo) return 0u;
  const CompactRun r = runs[lo - 1];
  return r.dst + (x - r.src < r.count ? x - r.src : r.count);
}
void launch_compact_planes(hipStream_t st, const CompactArgs& a, int compute_units);
// ... and beside it: the instance-level slot `src` (n16 pieces of 16 B) copied to both slots of the new allocation, the vertex, primitive
// and node_offset words of the n_instances DInstance records that begin at piece `first16` rebased by the same runs
void launch_compact_instances(hipStream_t st, uint4* dst0, uint4* dst1, const uint4* src, size_t n16, size_t first16, uint32_t n_instances, const CompactArgs& a);
// hk_add_meshes: n_prims HkPrimitive (48 B) and n_verts HkVertex (32 B) records - in pinned memory, or in the device block
// hk_add_meshes_device assembled them into - into the triangle planes and the vertex planes, from element 0 of the plane pointers given
void launch_append_geometry(hipStream_t st, const uint4* prims, uint32_t n_prims, const uint4* verts, uint32_t n_verts, float4* v0, float4* v1, float4* v2, float4* vn,
                            float2* vuv);
// hk_add_meshes_device: the HkPrimitive / HkVertex records of every source assembled from the caller's device memory in ONE launch of
// n_blocks workgroups whatever the number of sources (`items`, `blocks`: pinned; the first n_tri_blocks workgroups take triangles, the
// others vertices).  Values move as bits.  An index >= n_vertices reads vertex 0 instead and atomicMin-s the source's number into *status
// (device memory, HK_U32_MAX beforehand).  `sources_read` (or NULL) is recorded behind it.  Returns the kernels it launched.
uint32_t launch_assemble_meshes(hipStream_t st, const hkd::MeshSourceItem* items, const hkd::SegmentBlock* blocks, uint32_t n_tri_blocks, uint32_t n_blocks, uint32_t* status,
                                hipEvent_t sources_read);
void launch_gather_instance_boxes(hipStream_t st, const hkd::RefitScene& s, const float4* tlas, uint32_t tlas_count);
// the first n_emitter_updates records are the moved emitters (the largest of their meshes has emitter_triangles triangles)
void launch_refit(hipStream_t st, const hkd::RefitScene& s, const hkd::RefitUpdate* updates, uint32_t n_updates, uint32_t n_emitter_updates, uint32_t emitter_triangles,
                  uint32_t* failed, float4* tlas,
                  uint32_t tlas_count, uint32_t orderings, float4* light_lo, float4* light_hi, uint32_t light_count);
// hk_set_instance_transforms_device: the `moved` flags of all n_instances cleared and *status (or NULL) zeroed, then one RefitUpdate per
// named[r] = (instance, index of its pose at models + index * stride; DEVICE memory) into records[r] for launch_refit - moved 1 where the
// pose differs bit for bit from the model the device holds and can be inverted, else 0, with 1 + the instance id of an unusable pose
// atomicMax-ed into *status.  mesh_boxes: 2 float4 per instance (Aabb centre, half extents).  `sources_read` (or NULL) is recorded
// behind the launch that reads `models`.  Two launches whatever n_named is (one with none named); returns how many.
uint32_t launch_pose_records(hipStream_t st, const hkd::RefitScene& s, uint32_t n_instances, const uint2* named, uint32_t n_named, const void* models, uint32_t stride,
                             const float4* mesh_boxes, hkd::RefitUpdate* records, uint32_t* status, hipEvent_t sources_read);
// hk_update_materials: the changed records into `materials` (the slot's array, which s.materials names too), then - n_emitters != 0 -
// position_radius of the listed emitters again from their instances' boxes, and the light tree refit in its shape
void launch_material_update(hipStream_t st, const hkd::RefitScene& s, float4* materials, const hkd::MaterialUpdate* updates, uint32_t n_updates, const uint32_t* emitters,
                            uint32_t n_emitters, float4* light_lo, float4* light_hi, uint32_t light_count);
// hk_update_texture: n texels from pinned memory to their place in the texel buffer, and the texture's descriptor into `info0` / `info1` (or NULL)
void launch_texture_update(hipStream_t st, uint32_t* dst, const uint32_t* src, size_t n, uint4* info0, uint4* info1, uint4 info);
// hk_update_textures_device: every item's rectangle converted from the caller's memory into the texel buffer and every item's descriptor
// into info0[index] / info1[index] (or NULL), in ONE launch of n_blocks workgroups whatever the number of items (`items`, `blocks`: pinned).
// `thresholds`: 256 floats in device memory (hk_internal.hpp srgb_encode_thresholds).  `sources_read` (or NULL) is recorded behind it.
// Returns the kernels it launched.
uint32_t launch_textures_update(hipStream_t st, uint32_t* tex_data, const hkd::TextureItem* items, const hkd::SegmentBlock* blocks, uint32_t n_blocks,
                                const float* thresholds, uint4* info0, uint4* info1, hipEvent_t sources_read);
// A new tree over n shapes, built on the device into a flat skip-link BVH (kernels_tree.hip): the scratch one build needs in either
// mode, and the build
size_t lbvh_scratch_bytes(uint32_t n);
struct TreeBuild {
  int mode = 0;                            // 0 LBVH (Morton order), 1 the reference's binned SAH
  uint32_t n = 0;                          // shapes
  // the shapes: their boxes, or - box_lo == nullptr, the light tree - the emitters of `scene` (position -/+ radius)
  const float4 *box_lo = nullptr, *box_hi = nullptr;
  const hkd::RefitScene* scene = nullptr;
  // the node array to overwrite: `stride` float4 between consecutive nodes (2: interleaved lo / hi pairs, 1: two planes), `ord_stride`
  // float4 between orderings (0: the tree's own 3n - 2 nodes)
  float4 *lo = nullptr, *hi = nullptr;
  uint32_t stride = 2, orderings = 1;
  size_t ord_stride = 0;
  bool mesh_tree = false;                  // a mesh tree: ordering 0 stays left before right in either mode, the SAH top may take the whole chip
  const hkd::MeshTree* keep = nullptr;     // a mesh tree (mesh_tree must be set) that takes the new topology over, for its later refits
  bool one_workgroup_top = false;          // the SAH build's top levels in one workgroup at any n (A/B)
  void* scratch = nullptr;                 // lbvh_scratch_bytes(n)
  uint32_t* launches = nullptr;            // the kernel launches of the build are added to it
};
int launch_tree_build(hipStream_t st, const TreeBuild& d);
// The trees of MANY meshes in one build (`nodes` = the mesh-level node array, interleaved lo / hi pairs, `ord_stride` float4 between its
// orderings): the number of launches does not depend on the number of meshes.  Every mesh below hkd's SAH_WIDE_MIN triangles.
size_t forest_scratch_bytes(uint32_t n_tris, uint32_t n_meshes, int mode);
int launch_forest_build(hipStream_t st, int mode /* 0 LBVH, 1 the reference's binned SAH */, const hkd::ForestMesh* meshes /* host */, uint32_t n_meshes, uint32_t n_tris,
                        const float4* v0, const float4* v1, const float4* v2, void* scratch, float4* nodes, uint32_t orderings, size_t ord_stride, uint32_t* launches);
constexpr uint32_t HK_FOREST_MESH_MAX_TRIANGLES = 32767u;  // (SAH_WIDE_MIN - 1: from there a mesh has the whole chip to itself)
// mesh deformation: the BLAS refit of one mesh tree into `orderings` orderings of its flat layout (`lo` = its node 0 of ordering 0,
// interleaved lo / hi pairs, `ord_stride` float4 between orderings); the propagation of the new mesh boxes (6 order-preserving words
// each, kernels_deform.hip) to the instances of ALL the deformed meshes in one launch (`entries`: pinned, one per instance), their
// emitters (`records`: device scratch, one per emitting instance; the largest such mesh has emitter_triangles triangles) and both
// trees.  Returns the kernels it launched.
void launch_mesh_tree_refit(hipStream_t st, const hkd::MeshTree& t, float4* lo, size_t ord_stride, uint32_t orderings);
uint32_t launch_mesh_propagate(hipStream_t st, const hkd::RefitScene& s, const hkd::MeshInstanceEntry* entries, uint32_t n_entries, hkd::RefitUpdate* records,
                               uint32_t n_emitters, uint32_t emitter_triangles, float4* tlas, uint32_t tlas_count, uint32_t orderings, float4* light_lo, float4* light_hi,
                               uint32_t light_count);
// hk_change_scene_instances: the device's values over a freshly laid-out instance level `s` - the poses of the survivors from
// `old_instances` (or NULL: the host's poses stand), every instance's world box and emitter slot (into `emissive_of_instance`, the
// array s names), every emitter's record, surface area and alias slice (`records`: device scratch, one per emitter), then a refit of the
// trees given a node count (the single-leaf trees nothing builds).  `entries`: pinned, one per instance.  The launches do not follow
// the number of instances; returns how many.
uint32_t launch_instance_change(hipStream_t st, const hkd::RefitScene& s, uint32_t* emissive_of_instance, const hkd::DInstance* old_instances,
                                const hkd::InstanceDerive* entries, uint32_t n_instances, hkd::RefitUpdate* records, uint32_t n_emitters, uint32_t emitter_triangles,
                                float4* tlas, uint32_t tlas_count, uint32_t orderings, float4* light_lo, float4* light_hi, uint32_t light_count);
// hk_deform_meshes: `items` and the three workgroup tables (vertices, triangles = leaves, tree nodes x orderings) lie in pinned memory.
// Five launches whatever n_items is: begin (box words, joint palettes), vertices, triangles (+ arrival counters), boxes bottom-up, emit.
// hk_deform_meshes_device: `sources_read` (or NULL) is recorded behind the vertex launch, the last that reads the caller's memory; with
// n_normal_blocks (the vertex workgroups of the items that recompute their normals) a sixth launch gathers them behind the triangles.
void launch_deform_batch(hipStream_t st, const hkd::DeformItem* items, uint32_t n_items, const hkd::SegmentBlock* vertex_blocks, uint32_t n_vertex_blocks,
                         const hkd::SegmentBlock* triangle_blocks, uint32_t n_triangle_blocks, const hkd::SegmentBlock* node_blocks, uint32_t n_node_blocks,
                         size_t ord_stride, uint32_t orderings, hipEvent_t sources_read = nullptr, const hkd::SegmentBlock* normal_blocks = nullptr,
                         uint32_t n_normal_blocks = 0);
void launch_deform_tree_refit(hipStream_t st, const hkd::DeformItem* items, const hkd::SegmentBlock* triangle_blocks, uint32_t n_triangle_blocks,
                              const hkd::SegmentBlock* node_blocks, uint32_t n_node_blocks, size_t ord_stride, uint32_t orderings);  // (the last two of them: kernels_tree.hip)
void launch_mesh_stage(hipStream_t st, const float* positions, const float* normals, uint32_t n, float4* pos, float4* vn, uint32_t* box);
void launch_mesh_skin(hipStream_t st, const float4* bind_pos, const float4* bind_nrm, const uint2* joints, const float4* weights, const float4* joint_mats, uint32_t n,
                      float4* pos, float4* vn, uint32_t* box);
void launch_mesh_triangles(hipStream_t st, const float4* pos, float4* v0, float4* v1, float4* v2, uint32_t n_tris, float4* tri_lo, float4* tri_hi);
// the triangle boxes alone, from the triangle planes as they are (a mesh rebuilt before its first deformation)
void launch_mesh_triangle_boxes(hipStream_t st, const float4* v0, const float4* v1, const float4* v2, uint32_t n_tris, float4* tri_lo, float4* tri_hi);
// windowed: 0 the plain form, 1 the windowed form (depth window + tap lists in LDS: kernels.hip), -1 by the size of the launch; returns
// whether the windowed form was launched.  known: the table of the background's known records (launch_spatial_known_fill), or nullptr -
// the launch then takes the long way for every background tile, and its windowed form is handed no empty-tile / kept-tile plane
// (HK_DEBUG_OPT_SPATIAL_KNOWN 0: the A/B arm)
bool launch_spatial(hipStream_t st, bool emissive_lit, const hkd::DScene& sc, const hkd::DFrame& fr, const hkd::GBuffer& g, const hkd::LightTargets& t,
                    int y0, int y1, int windowed, const hkd::SpatialKnown* known, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);  // (events attached to the dispatch: HkStats timing)
void launch_spatial_known_fill(hipStream_t st, hkd::SpatialKnown* table);  // one wave; the table is complete once `st` has run it
void launch_derive_planes(hipStream_t st, const hkd::GBuffer& g, float* depth_plane, void* dn_g, int width, int y0, int y1);
void launch_count_geometry_rows(hipStream_t st, const float* depth, int width, int height, uint32_t* out);
void launch_demodulation(hipStream_t st, int nch, const hkd::DFrame& fr, const hkd::DemodTargets& d, int y0, int y1);
void launch_denoise(hipStream_t st, int level, int nch, int ffmask, const hkd::DFrame& fr, const hkd::DenoiseTargets& d, int y0, int y1);
void launch_tone_mapping(hipStream_t st, const hkd::DFrame& fr, const void* direct, const void* emissive, const void* indirect, void* out, int y0, int y1);
// anti-aliasing tail (kernels_aa.hip): raw plane pointers + sizes of one dispatch's bindings
struct AaBuffers {
  const void *position, *velocity_uv, *previous_position, *previous_velocity_uv, *instance_material;  // full size
  const float *depth, *previous_depth;  // position.w / previous_position.w alone: the depth-only taps read 4 B instead of 16
  int full_w, full_h;
  const void* render;           // rgba16f: tone_mapping_output[current] (SMAA) / TAA input
  int render_w, render_h;
  const void* previous_render;  // rgba16f: tone_mapping_output[previous] (SMAA) / taa_output[previous] (TAA)
  int previous_w, previous_h;
  void* output;                 // rgba16f
  int out_w, out_h;
};
// depth[i] = position[i].w of `pixels` rgba32f texels: the depth plane of a position plane the HOST wrote (the previous frame's)
void launch_depth_of_position(hipStream_t st, const void* position, float* depth, int pixels);
void launch_smaa_tu4x(hipStream_t st, const AaBuffers& b, uint32_t frame_number, int y0, int y1);
void launch_smaa_tu4x_extrapolate(hipStream_t st, void* output, int out_w, int out_h, int render_w, int y0, int y1);
void launch_taa_jasmine(hipStream_t st, const AaBuffers& b, float blend, const float clear_color[4], int y0, int y1);
void launch_fsr_easu(hipStream_t st, const void* input, int in_w, int in_h, void* output, int out_w, int out_h, int y0, int y1);
void launch_fsr_rcas(hipStream_t st, const void* input, void* output, int w, int h, float sharpness, int y0, int y1);
// hk_present: rows [y0, y1) of the host's target from the final image and the albedo (rgba16f planes of their own sizes)
void launch_present(hipStream_t st, const void* src, int src_w, int src_h, const void* albedo, int albedo_w, int albedo_h, const float* srgb_lut,
                    const HkPresentTarget& t, int y0, int y1);
// hk_cast_rays: n host rays (HkRay) -> n records (HkRayHit), both in device memory; flags = HK_RAYS_*; wide = the records of the wide
// walk (tlas and spill != nullptr, wide_lanes = the lanes the spill area serves) where closest hits of a scene in global memory are to
// take it, or nullptr (kernels_query.hip)
void launch_cast_rays(hipStream_t st, const hkd::DScene& sc, const hkd::WideTrees* wide, size_t wide_lanes, const void* rays, uint32_t n, uint32_t flags, void* hits);
// apply the parked scatter stores of pixels [p0, p1); [own0, own1) = the pixels this context dispatched itself (their winners are
// in), empty = all of them
void launch_resolve_scatter(hipStream_t st, const hkd::LightTargets& t, int p0, int p1, int own0, int own1);
// the light form (LightTargets::det_lite): rows [y0, y1) of the pass that just ran; `indirect`: the pass was indirect_lit_ambient (whose
// pixels are background also when the frame has no bounces, light.wgsl:1279)
void launch_resolve_scatter_lite(hipStream_t st, const hkd::LightTargets& t, const hkd::DFrame& fr, const float* depth_plane, bool indirect, int y0, int y1);
void launch_debug_math(hipStream_t st, uint32_t op, const float* x, const float* y, float* out, size_t n);
}  // namespace hk
