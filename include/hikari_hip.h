/*
 * hikari_hip.h - C ABI of libhikari_hip.so, the MI355X-native (HIP / gfx950) replacement for the
 * compute path of cryscan/bevy-hikari v0.3.15 (reference paths below are relative to that repo).
 *
 * What this boundary replaces
 * ---------------------------
 * In the reference the path sits behind three Bevy render-graph nodes that record wgpu compute /
 * raster work:  PrepassNode::run (src/prepass.rs:769-852), LightNode::run (src/light.rs:590-702)
 * and PostProcessNode::run (src/post_process.rs:1140-1234, denoise + tone mapping part).  Their
 * inputs are the storage buffers written in the Prepare stage (src/mesh_material/mesh.rs:43-64,
 * material.rs:139-203, instance.rs:82-108), the noise images (src/lib.rs:189-219) and the four
 * dynamic uniforms (src/prepass.rs:546-553).  A Rust `HikariPlugin` keeps all of that host code
 * and calls the functions below instead of creating wgpu pipelines (see INTEGRATION.md for the
 * `extern "C"` block).
 *
 * Conventions
 * -----------
 *  - plain C, no C++/torch types; every function returns HK_OK (0) or a negative HK_E* code and
 *    never throws.  The reference's nodes silently return Ok(()) when a resource is missing
 *    (light.rs:606-617); here the same situation is reported as HK_E_NOT_READY and nothing runs.
 *  - the library owns all device memory.  Host arrays passed to hk_upload_* are copied before
 *    the call returns.
 *  - one hk_ctx is bound to one HIP device and is used from one host thread at a time (Bevy runs
 *    the render graph sequentially on the render thread).  All kernels are enqueued on the
 *    context's HIP stream; hk_frame_wait() is the only synchronisation point.
 *  - Hk* data structs are byte-for-byte the std430 / std140 layouts the reference writes with
 *    encase (src/mesh_material/mod.rs:60-299, src/view.rs:105-123) so the Rust side can hand over
 *    its existing buffers unchanged.  Conversion to the device layout happens inside hk_upload_*.
 */
#ifndef HIKARI_HIP_H
#define HIKARI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libhikari_hip.so is built with -fvisibility=hidden (tools/build_lib.py): the entry points declared between this push and the pop at
 * the end of the header - and the hooks of hikari_hip_debug.h - are ALL it exports; a host that links it sees no internal symbol. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define HK_ABI_VERSION 8

/* ------------------------------------------------------------------ error codes */
#define HK_OK 0
#define HK_E_INVALID (-1)    /* bad argument (NULL, size mismatch, out-of-range enum) */
#define HK_E_NO_DEVICE (-2)  /* no HIP device / device id out of range */
#define HK_E_HIP (-3)        /* a HIP runtime call failed; see hk_last_error() */
#define HK_E_NOT_READY (-4)  /* scene / noise / size / uniforms not uploaded yet */
#define HK_E_NOMEM (-5)
#define HK_E_UNSUPPORTED (-6)

/* ------------------------------------------------------------------ scene data (std430) */

/* mesh_material_types.wgsl:3-8, mod.rs:67-73 (GpuVertexCompact), 32 B */
typedef struct HkVertex {
  float position[3];
  float u;
  float normal[3];
  float v;
} HkVertex;

/* mesh_material_types.wgsl:10-17, mod.rs:115-145 (GpuPrimitiveCompact), 48 B */
typedef struct HkPrimitiveVertex {
  float position[3];
  uint32_t index;
} HkPrimitiveVertex;
typedef struct HkPrimitive {
  HkPrimitiveVertex vertices[3];
} HkPrimitive;

/* mesh_material_types.wgsl:35-40, mod.rs:177-201 (GpuNode), 32 B.
 * Skip-link flat BVH node.  entry_index >= 0x80000000 marks a leaf (low bits = shape index);
 * leaf boxes are EMPTY (min=+inf, max=-inf) exactly as `bvh` 0.7.1 flatten_custom emits them. */
typedef struct HkNode {
  float min[3];
  uint32_t entry_index;
  float max[3];
  uint32_t exit_index;
} HkNode;
#define HK_BVH_LEAF_FLAG 0x80000000u

/* mesh_material_types.wgsl:19-23, mod.rs:469-476 (GpuMeshIndex), 16 B */
typedef struct HkMeshIndex {
  uint32_t vertex;
  uint32_t primitive;
  uint32_t node_offset;
  uint32_t node_count;
} HkMeshIndex;
/* A mesh's three ranges in the concatenated arrays of the builder's LAST finish (hk_scene_builder_remove_mesh, hk_remove_meshes), 24 B.
 * n_primitives is the triangle count, node_count = 3 n_primitives - 2; node_count 0: a mesh no finish has seen (it lies in no array). */
typedef struct HkMeshExtent {
  uint32_t vertex, n_vertices;
  uint32_t primitive, n_primitives;
  uint32_t node_offset, node_count;
} HkMeshExtent;

/* mesh_material_types.wgsl:25-33, mod.rs:147-156 (GpuInstance), 176 B. Matrices column-major. */
typedef struct HkInstance {
  float min[3];
  uint32_t material;
  float max[3];
  uint32_t node_index;
  float model[16];
  float inverse_transpose_model[16];
  HkMeshIndex mesh;
} HkInstance;

/* mesh_material_types.wgsl:42-56, mod.rs:203-218 (GpuStandardMaterial), 80 B */
typedef struct HkMaterial {
  float base_color[4];
  uint32_t base_color_texture;
  uint32_t _pad0[3];
  float emissive[4];
  uint32_t emissive_texture;
  float perceptual_roughness;
  float metallic;
  uint32_t metallic_roughness_texture;
  float reflectance;
  uint32_t normal_map_texture;
  uint32_t occlusion_texture;
  uint32_t _pad1;
} HkMaterial;
#define HK_NO_TEXTURE 0xFFFFFFFFu

/* mesh_material_types.wgsl:58-61, mod.rs:220-226, 8 B */
typedef struct HkAliasEntry {
  float prob;
  uint32_t index;
} HkAliasEntry;

/* mesh_material_types.wgsl:63-71, mod.rs:228-237 (GpuEmissive), 64 B */
typedef struct HkEmissive {
  float emissive[4];
  float position[3];
  float radius;
  uint32_t instance;
  uint32_t _pad0;
  uint32_t alias_table[2]; /* x = offset, y = count */
  float surface_area;
  uint32_t node_index;
  uint32_t _pad1[2];
} HkEmissive;

/* ------------------------------------------------------------------ uniforms */

/* mesh_view_types.wgsl:3-20, view.rs:105-123 (FrameUniform), std140: 244 B -> 256 B */
typedef struct HkFrame {
  float kernel[3][4]; /* mat3x3, each column padded to vec4 */
  float halton[8][4];
  float clear_color[4];
  uint32_t number;
  uint32_t direct_validate_interval;
  uint32_t emissive_validate_interval;
  uint32_t indirect_bounces;
  uint32_t temporal_reuse;
  uint32_t emissive_spatial_reuse;
  uint32_t indirect_spatial_reuse;
  uint32_t max_temporal_reuse_count;
  uint32_t max_spatial_reuse_count;
  float max_reservoir_lifetime;
  float solar_angle;
  float max_indirect_luminance;
  float upscale_ratio;
  uint32_t _pad[3];
} HkFrame;

/* bevy_pbr 0.9.1 `View` uniform (bevy_pbr::mesh_view_types; used at light.wgsl:721-724,1040 and
 * prepass.wgsl:45,71,96).  Matrices column-major. 416 B. */
typedef struct HkView {
  float view_proj[16];
  float inverse_view_proj[16];
  float view[16];
  float inverse_view[16];
  float projection[16];
  float inverse_projection[16];
  float world_position[3];
  float _pad0;
  float viewport[4]; /* x, y, width, height in physical pixels */
} HkView;

/* mesh_view_types.wgsl:22-25, view.rs:31-35 (PreviousViewUniform), 128 B */
typedef struct HkPreviousView {
  float view_proj[16];
  float inverse_view_proj[16];
} HkPreviousView;

/* The three fields of bevy_pbr 0.9.1 `Lights` the path reads (light.wgsl:611,832,847-855):
 * directional_lights[0].{color, direction_to_light} and ambient_color.  With no directional light
 * bevy zero-fills entry 0; pass n_directional_lights = 0 and zeros to reproduce that. */
typedef struct HkLights {
  float directional_color[4];
  float direction_to_light[3];
  uint32_t n_directional_lights;
  float ambient_color[4];
} HkLights;

/* HikariSettings (src/lib.rs:400-455), field for field.  hk_settings_default() fills the
 * reference defaults (lib.rs:435-455). */
typedef enum HkTaa { HK_TAA_JASMINE = 0, HK_TAA_NONE = 1 } HkTaa;           /* lib.rs:466-472 */
typedef enum HkUpscaleKind { HK_UPSCALE_FSR1 = 0, HK_UPSCALE_SMAA_TU4X = 1 } HkUpscaleKind; /* lib.rs:474-487 */
typedef struct HkSettings {
  uint32_t direct_validate_interval;
  uint32_t emissive_validate_interval;
  uint32_t max_temporal_reuse_count;
  uint32_t max_spatial_reuse_count;
  float max_reservoir_lifetime;
  float solar_angle;
  uint32_t indirect_bounces;
  float max_indirect_luminance;
  float clear_color[4];
  uint32_t temporal_reuse;
  uint32_t emissive_spatial_reuse;
  uint32_t indirect_spatial_reuse;
  uint32_t denoise;
  uint32_t taa;           /* HkTaa */
  uint32_t upscale_kind;  /* HkUpscaleKind */
  float upscale_ratio;    /* clamped to [1,2] like Upscale::ratio(), lib.rs:500-504 */
  float upscale_sharpness;
} HkSettings;

/* ------------------------------------------------------------------ buffers & passes */

/* Screen-space resources (group 1, 5, 6 of the light pipeline and group 3/4 of the denoise
 * pipeline: deferred_bindings.wgsl:3-20, light.wgsl:26-31,68-75, denoise.wgsl:10-28). Formats are
 * the reference's texture formats flattened row-major (prepass.rs:43-47, light.rs:29-31,
 * post_process.rs:29): rgba32f = 16 B, rgba8snorm = 4 B, rg32f = 8 B, rgba16f = 8 B, r32f = 4 B,
 * PackedReservoir = 64 B (light.wgsl:35-43). */
typedef enum HkBuffer {
  HK_BUF_POSITION = 0,          /* rgba32f, full size: world xyz, w = clip depth (0 = background) */
  HK_BUF_NORMAL = 1,            /* rgba8snorm, full */
  HK_BUF_DEPTH_GRADIENT = 2,    /* rg32f, full */
  HK_BUF_INSTANCE_MATERIAL = 3, /* rg32f (id + 0.5), full */
  HK_BUF_VELOCITY_UV = 4,       /* rgba32f, full */
  HK_BUF_ALBEDO = 5,            /* rgba16f, full */
  HK_BUF_VARIANCE0 = 6,         /* r32f, scaled; +channel (0 sun, 1 emissive, 2 indirect) */
  HK_BUF_RENDER0 = 9,           /* rgba16f, scaled; +channel */
  HK_BUF_RESERVOIR0 = 12,       /* 64 B x full W*H; +k, k in 0..9 (light.rs:342-363) */
  HK_BUF_DENOISE_INTERNAL0 = 22,/* rgba16f, scaled; +level 0..3 */
  HK_BUF_DENOISE_INTERNAL_VARIANCE = 26, /* r32f, scaled */
  HK_BUF_DENOISE_RENDER0 = 27,  /* rgba16f, scaled; +channel */
  HK_BUF_TONE_MAPPED = 30,      /* rgba16f, scaled (tone_mapping.wgsl:21-32): tone_mapping_output[current] */
  /* Temporal anti-aliasing / upscale inputs and outputs (post_process.rs:621-748, prepass.rs:285-318).
   * The reference double-buffers these by frame: position / velocity_uv swap every frame
   * (prepass.rs:308-317), tone_mapping_output and taa_output are indexed by frame.number % 2
   * (post_process.rs:737,866-867).  Here all four follow frame.number % 2 of hk_frame_begin: ids
   * without PREVIOUS name the plane frame n writes, PREVIOUS_* the plane frame n-1 wrote.
   * hk_device_ptr of these ids is therefore only valid until the next hk_frame_begin, and a host
   * that supplies its own G-buffer writes it AFTER hk_frame_begin of that frame.
   * Since ABI 6 the same holds for HK_BUF_ALBEDO and HK_BUF_DEPTH_GRADIENT (no PREVIOUS ids: nothing reads last frame's): the
   * a-trous levels of frame n may still be reading them on their own stream while frame n + 1's primary rays write the other
   * parity's planes (frame pipelining; contexts created with HK_CTX_SINGLE_STREAM / _DETERMINISTIC_SCATTER / _COUNT_RAYS /
   * _TIME_PASSES keep one plane).  hk_read_buffer / hk_write_buffer always address the current frame's plane. */
  HK_BUF_PREVIOUS_POSITION = 31,
  HK_BUF_PREVIOUS_VELOCITY_UV = 32,
  HK_BUF_PREVIOUS_TONE_MAPPED = 33,
  HK_BUF_UPSCALE_OUTPUT = 34,   /* rgba16f, ceil(size * 2 / ratio): upscale_output[0] of the SMAA Tu4x path */
  HK_BUF_TAA_OUTPUT = 35,       /* rgba16f: taa_output[current]; size of UPSCALE_OUTPUT (SMAA) or scaled (FSR1) */
  HK_BUF_PREVIOUS_TAA_OUTPUT = 36,
  /* FSR1 (Upscale::Fsr1): upscale_output[0] (EASU result) is HK_BUF_UPSCALE_OUTPUT at the window size, upscale_output[1]
   * (RCAS result, what OverlayNode presents, overlay.rs:228) is this one: rgba16f, window size */
  HK_BUF_UPSCALE_SHARPENED = 37,
  /* Parked scatter stores (ABI 7).  A temporal dispatch stores a rejected history reservoir at the REPROJECTED
   * pixel of previous_spatial (light.wgsl:1063,1092-1095,1199-1202,1456-1459) - a slot some other thread, possibly some other
   * BAND, owns.  Where those stores are parked instead of raced (HK_CTX_DETERMINISTIC_SCATTER, and every band of a sharded frame
   * whose history halo is not empty) pixel i of channel c (0 sun, 1 emissive, 2 indirect) leaves the slot it stores to in
   * PARKED_TO0 + c (i32 per render pixel, -1 = no store) and the 64-B record in PARKED_RECORD0 + c; the highest pixel index that
   * stores to a slot wins.  Rows of these planes are what bands hand each other with exchange A under motion
   * (HK_STAGE_SPATIAL_WITH_HISTORY).  Allocated on first use: hk_device_ptr / hk_read_buffer fail with HK_E_INVALID before. */
  HK_BUF_PARKED_TO0 = 38,       /* i32, scaled; +channel */
  HK_BUF_PARKED_RECORD0 = 41,   /* 64 B, scaled; +channel */
  HK_BUF_COUNT = 44
} HkBuffer;

/* One compute dispatch of the reference.  `arg` selects the render channel for
 * the denoise passes and the a-trous level is part of the pass id. */
typedef enum HkPass {
  HK_PASS_PREPASS = 0,             /* prepass.wgsl:40-100 semantics, produced by primary rays */
  HK_PASS_FULL_SCREEN_ALBEDO = 1,  /* light.wgsl:1019-1042 */
  HK_PASS_DIRECT_LIT = 2,          /* light.wgsl:1044-1261, RENDER_EMISSIVE (sun) */
  HK_PASS_DIRECT_EMISSIVE = 3,     /* light.wgsl:1044-1261, EMISSIVE_LIT */
  HK_PASS_INDIRECT = 4,            /* light.wgsl:1263-1498; MULTIPLE_BOUNCES iff bounces >= 2 (light.rs:663-666) */
  HK_PASS_EMISSIVE_SPATIAL_REUSE = 5, /* light.wgsl:1503-1684, EMISSIVE_LIT */
  HK_PASS_INDIRECT_SPATIAL_REUSE = 6, /* light.wgsl:1503-1684 */
  HK_PASS_DEMODULATION = 7,        /* denoise.wgsl:135-162; arg = channel */
  HK_PASS_DENOISE_L0 = 8,          /* denoise.wgsl:215-319; arg = channel; +level 0..3 */
  HK_PASS_DENOISE_L1 = 9,
  HK_PASS_DENOISE_L2 = 10,
  HK_PASS_DENOISE_L3 = 11,
  HK_PASS_TONE_MAPPING = 12,       /* tone_mapping.wgsl:21-32 */
  HK_PASS_SMAA_TU4X = 13,          /* smaa.wgsl:81-188: current + reprojected previous sample of each output quad */
  HK_PASS_SMAA_TU4X_EXTRAPOLATE = 14, /* smaa.wgsl:239-271: the other two pixels of each quad */
  HK_PASS_TAA_JASMINE = 15,        /* taa.wgsl:75-170 */
  HK_PASS_FSR_EASU = 16,           /* FidelityFX FSR 1.0 edge-adaptive spatial upsampling: src/shaders/fsr/source.zip,
                                      ffx_fsr1.h FsrEasuF through FSR_Pass.glsl (the blob fsr_pass_easu.spv), post_process.rs:1277-1293 */
  HK_PASS_FSR_RCAS = 17,           /* ... robust contrast-adaptive sharpening, FsrRcasF (fsr_pass_rcas.spv), post_process.rs:1295-1308 */
  HK_PASS_COUNT = 18
} HkPass;

/* Frame stages for band-sharded (multi-GPU) rendering: the host exchanges halo rows between
 * stages (hk_band_plan).  A single-GPU frame is the three stages back to back. */
typedef enum HkStage {
  HK_STAGE_TEMPORAL = 0,     /* prepass (+apron), albedo, direct_lit x2, indirect on the band */
  HK_STAGE_SPATIAL = 1,      /* spatial_reuse dispatches that are enabled */
  HK_STAGE_POST_PROCESS = 2, /* demodulation + a-trous x4 per channel, tone mapping */
  HK_STAGE_ANTIALIAS = 3,    /* the rest of PostProcessNode::run (post_process.rs:1236-1272): SMAA Tu4x (+extrapolate)
                                when upscale_kind is SMAA_TU4X, then TAA when taa is JASMINE, on the band (exchange D of
                                hk_band_plan_for: tone-mapped rows + last frame's TAA rows).  Not part of hk_frame_render
                                unless HK_FRAME_ANTIALIAS. */
  HK_STAGE_UPSCALE = 4,      /* upscale_kind FSR1 only (post_process.rs:1277-1308; a no-op for SMAA_TU4X): EASU + RCAS to the
                                window size.  A band owns the window rows hk_band_rows(height, ..) gives it: EASU runs on those
                                rows +-1 (RCAS's cross), RCAS on the rows themselves; exchange E of hk_band_plan_for brings the
                                3-4 rows of the EASU input (taa_output or tone-mapped) the 12 taps reach beyond the render band.
                                Runs after HK_STAGE_ANTIALIAS under HK_FRAME_ANTIALIAS. */
  HK_STAGE_COUNT = 5
} HkStage;

/* One halo transfer the host must perform BEFORE running `stage`: rows [row_begin,row_end) of
 * `buffer` (row = `row_bytes` bytes at device offset row*row_bytes) travel from the rank that owns
 * them to this rank.  peer = band index of the owner. */
typedef struct HkHaloOp {
  uint32_t buffer;     /* HkBuffer */
  uint32_t peer;       /* band index (= rank) that owns the rows */
  uint32_t row_begin;
  uint32_t row_end;
  uint64_t row_bytes;
} HkHaloOp;

#define HK_TIMING_SLOTS 24
/* slot 18 (beyond the HkPass ids): every TRACE launch of the queue-based indirect pass on its own (bounces + 1 launches per pass);
 * selected like a pass, by bit 18 of hk_set_timing_mask - and only so: HK_CTX_TIME_PASSES selects the HkPass slots 0 .. HK_PASS_COUNT - 1 */
#define HK_TIMING_TRACE_STAGES 18u
/* slot 19: the motion pass behind the primary rays (hk_set_mesh_motion_vectors), selected by bit 19 of hk_set_timing_mask alone */
#define HK_TIMING_MOTION_VECTORS 19u
typedef struct HkStats {
  uint64_t rays_primary;      /* G-buffer rays */
  uint64_t rays_tlas;         /* traverse_top invocations (light.wgsl:442) */
  uint64_t rays_blas;         /* stand-alone traverse_bottom invocations (light.wgsl:687) */
  uint64_t frames;
  /* HIP-event timing on the context's stream.  Slot = HkPass id.  Only passes selected by
   * hk_set_timing_mask() (every HkPass, with HK_CTX_TIME_PASSES) are bracketed by events. */
  double pass_ms_total[HK_TIMING_SLOTS];
  uint64_t pass_launches[HK_TIMING_SLOTS];
  float last_frame_ms;        /* first dispatch of TEMPORAL .. last dispatch of POST_PROCESS */
  uint32_t _pad;
  /* how often the device scene was (re)built since hk_create: the mesh-level arrays (BLAS nodes,
   * triangles, vertices) and the instance-level arrays (TLAS, instances, lights, materials).  An
   * instance-only update must leave scene_mesh_builds unchanged. */
  uint64_t scene_mesh_builds;
  uint64_t scene_instance_builds;
  /* ... of which the instance-level arrays went through pinned staging into the spare slot in stream order, with no
   * host or device wait (scenes larger than the 32 KB LDS copy keep two slots of the instance-level region) */
  uint64_t scene_async_instance_uploads;
  /* instance updates that ran on the device (hk_refit_scene_instances): no host tree build, no scene buffer over PCIe */
  uint64_t scene_device_refits;
  uint64_t scene_device_tree_builds;  /* hk_rebuild_scene_trees */
  /* ABI 7, HK_CTX_COUNT_RAYS: what the counted walks did, in the terms of SURVEY 8d's algorithmic BVH bytes per ray - node steps
   * (32 B each: two 16-B loads), triangle tests (48 B), instance entries (a 208-B record; the survey's formula leaves them out),
   * closest hits whose attributes were fetched (three 32-B vertex records).  bench.py prices the trace kernels of the large-scene
   * configs with them (roofline of extra_configs 3 / 4). */
  uint64_t walk_node_steps;
  uint64_t walk_triangle_tests;
  uint64_t walk_instance_entries;
  uint64_t walk_closest_hits;
  uint64_t walk_top_node_steps;  /* ... of walk_node_steps, those taken in the instance tree (the rest walk mesh trees) */
  /* The wide walk (HK_TRAVERSAL_WIDE) keeps a lane's pending subtrees on a stack of 124 entries (28 in LDS, 96 behind them): enough
   * for trees 80 levels deep.  An entry that did not fit is DROPPED - geometry behind it is not seen by that ray - and counted here
   * (every context counts, not only HK_CTX_COUNT_RAYS): a host that loads degenerate trees checks this for 0 after its first
   * frames and creates the context with HK_CTX_NO_WIDE_WALK otherwise.  0 in every test and benchmark of this repository. */
  uint64_t wide_stack_lost;
} HkStats;

typedef struct hk_ctx hk_ctx;

/* ------------------------------------------------------------------ lifetime */
uint32_t hk_abi_version(void);
const char* hk_last_error(void); /* thread-local description of the last failure */
/* What this binary was built from (tools/build_lib.py): "sources <sha256[:16] of csrc/ + include/> | <hipcc, its version, every flag> |
 * built <UTC time>".  A host (and __graft_entry__.smoke()) can tell a stale library from the tree it sits in. */
const char* hk_build_info(void);
int hk_device_count(int* count);
/* Creates a context on HIP device `device_id`; flags: bit0 = count rays (HK_CTX_COUNT_RAYS),
 * bit1 = time every dispatch with HIP events (HK_CTX_TIME_PASSES), bit2 = take every (k + 0.5) / size through
 * the IEEE division sequence instead of the certified 3-instruction route (HK_CTX_PLAIN_DIVISION; the results
 * are identical bit for bit, the flag exists so that tests can show it). */
#define HK_CTX_COUNT_RAYS 1u
#define HK_CTX_TIME_PASSES 2u
#define HK_CTX_PLAIN_DIVISION 4u
/* By default hk_frame_stage / hk_frame_render run the two direct-light dispatches (sun, emissive: light.rs:656-688)
 * on a second HIP stream, concurrently with indirect_lit_ambient and its spatial pass - they touch disjoint
 * reservoir / render buffers (light.rs:518-546) - and join before anything reads their outputs (demodulation, halo
 * exchange B, hk_read_buffer, hk_frame_wait ...).  hk_pass_run never forks.  bit3 keeps everything on one stream:
 * same results, no overlap (used to time a kernel alone). */
#define HK_CTX_SINGLE_STREAM 8u
/* Verification mode.  The reference lets the stores to previous_spatial_reservoir_buffer race under camera / object
 * motion (light.wgsl:1063,1092-1095,1199-1202,1456-1459: a thread stores at the REPROJECTED pixel, which another thread
 * owns); by default so does this library - same kernels, whichever store arrives last stays.  bit4 parks those stores and
 * applies them after the dispatch so that the store of the highest thread index wins, which is how the CPU oracle
 * resolves the race: with it a moving camera and moving objects are bit-exact against the oracle too.  Costs three
 * extra launches and 72 B per pixel of scratch per light dispatch; not meant for production frames. */
#define HK_CTX_DETERMINISTIC_SCATTER 16u
/* Round 6.  The rule above costs little in its light form - a store to the pixel's own slot goes straight to the buffer, only a store
 * to another pixel's slot is parked and weighed against the slot's owner afterwards (one small launch per channel; the uniform-tile
 * store elision and the frame pipelining stay on) - so a single context now applies it BY DEFAULT to the channels whose
 * previous_spatial buffer has a reader (the indirect channel when indirect_spatial_reuse is on, sun + emissive when
 * emissive_spatial_reuse is on): what is rendered no longer depends on which store lands last, and equals the oracle's frames under
 * motion.  HK_CTX_DETERMINISTIC_SCATTER extends it to all three channels (every reservoir byte reproducible);
 * HK_CTX_RACING_SCATTER (bit10) restores the reference's own race - the A/B of bench.py --motion. */
#define HK_CTX_RACING_SCATTER 1024u
/* Traversal order.  The reference walks its flat BVHs in ONE fixed depth-first order (`bvh` 0.7.1 flatten_custom: left child
 * first, light.wgsl:400-486), which for a closest-hit ray coming "from the right" means visiting most of the tree before the
 * near hit that would have pruned it.  For scenes too large for the LDS copy the library therefore keeps EIGHT flattenings of
 * every TLAS / BLAS - one per sign pattern of the ray direction, children ordered the way such a ray meets them
 * (hk_bvh_rethread) - and each ray walks the one of its octant with the same stackless loop: same nodes, boxes, leaves and
 * per-candidate arithmetic, so the closest hit is the reference's except where two candidates tie exactly (which the order
 * breaks differently) - parity is then the north star's 1e-3 relative L2, not bit equality.  Occlusion (any-hit) results do
 * not depend on the order at all.  bit5 forces the reference's single order everywhere: the verification mode in which large
 * scenes are bit-exact against the oracle too.  Scenes that fit the LDS copy (Cornell) always use the reference order. */
#define HK_CTX_EXACT_TRAVERSAL 32u
/* Schedule of indirect_lit_ambient with two or more bounces (light.wgsl:1263-1498, the MULTIPLE_BOUNCES pipeline of
 * light.rs:663-666).  FUSED: one kernel, one pixel per lane from the G-buffer read to the reservoir store - the walks of a
 * wave last as long as its slowest ray.  WAVEFRONT: the same per-pixel arithmetic cut at the walks - a set-up dispatch gives
 * every non-background pixel a path slot, persistent trace waves pull rays from a queue (a lane whose ray has ended takes the
 * next one: wave ballot + prefix count, one atomic per 64 rays), a shade dispatch per bounce emits that bounce's shadow ray and
 * the next closest-hit ray into one queue and compacts the surviving paths; path state travels in 16-B planes indexed by slot
 * (~290 B per pixel of scratch, allocated on first use).  Both schedules produce the same bytes in every buffer.  Default:
 * wavefront for scenes beyond the LDS copy (long walks, where lane refill pays), fused for scenes that fit it (short walks,
 * where the ~0.4 KB per path and bounce of queue traffic costs more than the idle lanes).  bit6 / bit7 force one or the other. */
#define HK_CTX_WAVEFRONT 64u
#define HK_CTX_FUSED_INDIRECT 128u
/* Scenes beyond the LDS copy, product default (no HK_CTX_EXACT_TRAVERSAL): the CLOSEST-HIT walks - the primary rays of the prepass and
 * every ray of the wavefront schedule's trace stages - read 128-B records of an inner node's four grandchildren (derived on the
 * device from ordering 0 of the trees the scene holds) and take the children nearest first with a per-lane stack: two levels of the
 * tree per dependent fetch, on both levels of the scene.  Same candidates, same per-triangle arithmetic on the same operands, and of
 * two candidates at EXACTLY the same distance the one the reference's own walk meets first (decided from the leaves' positions in
 * the reference's flattening, kept next to the records): the closest hit is the reference's - up to box culls that depend on the
 * visit order (the reference tests a leaf's own box against the closest distance at the moment it VISITS the leaf, light.wgsl:412,
 * the wide walk when it processes the parent record: where a box is grazed within rounding one of them tests a triangle the other
 * skips; measured <= 1 primary hit per 8.3 M pixels and <= 6.3e-5 relative L2 over 32 frames against HK_CTX_EXACT_TRAVERSAL,
 * profiles/r05_default_mode_sequence_config4_4k.json) -, independent of the visit order, of
 * timing, and of how the trace stage splits a long walk among the idle lanes of its wave at the end of a stage; two runs of the
 * same frames are equal byte for byte.  Any-hit rays: whether a ray is occluded does not depend on the order; the rays whose
 * OCCLUDER is kept (the direct-light passes store its position in the reservoir) walk the reference's own order.  bit8 switches the
 * wide walk off (the closest-hit walks then take the direction-threaded skip-link walk, whose exact ties may fall differently): the
 * A/B the tests and `bench.py --no-wide-walk` use.  hk_traversal_mode reports HK_TRAVERSAL_WIDE when it is in use;
 * HkStats.wide_stack_lost counts pending subtrees a walk had to drop (0 for trees up to ~80 levels deep). */
#define HK_CTX_NO_WIDE_WALK 256u
/* Measurement (round 5): the frame takes exactly the schedule and walks it takes without the flag - unlike HK_CTX_COUNT_RAYS, whose
 * counting kernels exist in the fused form only and switch the queue-based schedule off - but the trace stages of the queue-based
 * indirect pass run the COUNTING twin of their kernel: per stage, records fetched (of them in the instance tree), triangle tests,
 * instance entries, rays, closest hits, pieces of long walks handed to idle lanes, and the moments the stage's queue ran dry and its
 * last wave left (hikari_hip_debug.h hk_debug_read_wf_timeline).  bench.py prices the trace kernel of configs 3 / 4 with these - the
 * walk that is TIMED, not a replay in another form. */
#define HK_CTX_COUNT_WALKS 512u
int hk_create(int device_id, uint32_t flags, hk_ctx** out);
void hk_destroy(hk_ctx* ctx);

/* ------------------------------------------------------------------ host-side mirrors of reference logic (no GPU needed) */
int hk_settings_default(HkSettings* out);                                        /* lib.rs:435-455 */
/* FrameUniform::extract_component, view.rs:141-193 (+ KERNEL / HALTON consts view.rs:125-139) */
int hk_frame_from_settings(const HkSettings* settings, uint32_t frame_number, HkFrame* out);
/* scaled render size = ceil(size / ratio), light.rs:318-319,623-624 */
int hk_scaled_size(uint32_t width, uint32_t height, float upscale_ratio, uint32_t* sw, uint32_t* sh);

/* Scene builder: the Prepare-stage host work of the reference, re-implemented in C++.
 *   add_mesh      -> TryFrom<Mesh> for GpuMesh, mod.rs:379-467 (triangle list / strip rules,
 *                    BLAS via `bvh` 0.7.1 BVH::build + flatten_custom(GpuNode::pack))
 *   add_material  -> material.rs:168-199 (values are passed through unchanged)
 *   add_instance  -> instance.rs:286-325 (world AABB from the 8 transformed half-extent corners)
 *   finish        -> mesh.rs:106-166 (concatenate + offsets), instance.rs:352-428 (TLAS, emissive
 *                    list, per-instance alias tables mod.rs:330-376, light BVH)
 * Arrays returned by the getters stay valid until the builder is destroyed. */
typedef struct hk_scene_builder hk_scene_builder;
#define HK_TOPOLOGY_TRIANGLE_LIST 0u
#define HK_TOPOLOGY_TRIANGLE_STRIP 1u
int hk_scene_builder_create(hk_scene_builder** out);
void hk_scene_builder_destroy(hk_scene_builder* b);
int hk_scene_builder_add_mesh(hk_scene_builder* b, const float* positions, const float* normals, const float* uvs,
                              uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, uint32_t topology,
                              uint32_t* mesh_id);
int hk_scene_builder_add_material(hk_scene_builder* b, const HkMaterial* material, uint32_t* material_id);
int hk_scene_builder_add_instance(hk_scene_builder* b, uint32_t mesh_id, uint32_t material_id,
                                  const float transform[16], uint32_t* instance_id);
int hk_scene_builder_finish(hk_scene_builder* b);
/* hk_scene_builder_finish WITHOUT its two `BVH::build` calls (instance.rs:365-371,422-428): every per-instance and per-emitter
 * record as above, the instance tree and the light tree as cheap valid stand-ins (index list halved recursively) of the final
 * size - for hosts that let the device build the trees (hk_update_scene_instances). */
int hk_scene_builder_finish_instances(hk_scene_builder* b);
/* Instance set edits (the reference's prepare_instances runs again on any of them, instance.rs:352-437).  Removing an instance
 * shifts the ids of the instances added after it down by one; its transform history goes with it. */
int hk_scene_builder_remove_instance(hk_scene_builder* b, uint32_t instance_id);
int hk_scene_builder_set_instance_material(hk_scene_builder* b, uint32_t instance_id, uint32_t material_id);
/* New values for an existing material (Bevy: `materials.get_mut(handle)`, which makes prepare_instances run again, instance.rs:352-437).
 * Like hk_scene_builder_set_instance_material it un-finishes the builder at the instance level only - meshes and their trees are kept -
 * and the next finish gives exactly what a builder that had these values from the start gives (emitter radius, emitter list, alias
 * tables and light tree included).  HK_E_INVALID for NULL or an unknown id: the builder is unchanged and still finished if it was.
 * The device path of the same edit is hk_update_materials. */
int hk_scene_builder_set_material(hk_scene_builder* b, uint32_t material_id, const HkMaterial* material);
/* Dynamic scenes (instance.rs:352-437 re-runs whenever an instance changes): replace an instance's
 * transform after a finish; the next finish redoes only the instance-level work (world AABBs, TLAS,
 * emissive list, alias tables, light BVH) - meshes and their BLAS are kept.  The transform the
 * instance had at the previous finish becomes its "previous transform" (PreviousMeshUniform,
 * instance.rs:111-128), which the G-buffer's velocity output needs. */
int hk_scene_builder_set_instance_transform(hk_scene_builder* b, uint32_t instance_id, const float transform[16]);
/* n instances x 16 floats (column-major): each instance's transform at the finish before the last one */
int hk_scene_builder_previous_transforms(const hk_scene_builder* b, const float** p, uint32_t* n);
int hk_scene_builder_vertices(const hk_scene_builder* b, const HkVertex** p, uint32_t* n);
int hk_scene_builder_primitives(const hk_scene_builder* b, const HkPrimitive** p, uint32_t* n);
int hk_scene_builder_asset_nodes(const hk_scene_builder* b, const HkNode** p, uint32_t* n);
int hk_scene_builder_materials(const hk_scene_builder* b, const HkMaterial** p, uint32_t* n);
int hk_scene_builder_instances(const hk_scene_builder* b, const HkInstance** p, uint32_t* n);
int hk_scene_builder_instance_nodes(const hk_scene_builder* b, const HkNode** p, uint32_t* n);
int hk_scene_builder_emissives(const hk_scene_builder* b, const HkEmissive** p, uint32_t* n);
int hk_scene_builder_emissive_nodes(const hk_scene_builder* b, const HkNode** p, uint32_t* n);
int hk_scene_builder_alias_table(const hk_scene_builder* b, const HkAliasEntry** p, uint32_t* n);
/* The host twin of hk_update_mesh_vertices: new positions (n_vertices x 3 floats, the mesh's own count) and normals (or NULL: keep)
 * of a finished mesh.  Topology and tree links are kept; every tree box becomes the union of the triangle boxes below it (what the
 * device refit computes), the mesh box is re-derived.  The next finish lays the instance level out again from them. */
int hk_scene_builder_set_mesh_vertices(hk_scene_builder* b, uint32_t mesh_id, const float* positions, const float* normals);
/* The host twin of HK_DEFORM_RECOMPUTE_NORMALS (hk_deform_meshes_device): the mesh's vertex normals rewritten from its CURRENT
 * positions by the same rule in the same f32 arithmetic - area-weighted face vectors summed per vertex in ascending triangle, then
 * corner order; a vertex whose sum is all zero keeps its normal.  Like hk_scene_builder_set_mesh_vertices it un-finishes the mesh
 * level; an unknown id returns HK_E_INVALID with the builder unchanged.  set_mesh_vertices(positions, NULL) and then this call bring
 * the host's mirror back after such a device deformation. */
int hk_scene_builder_recompute_mesh_normals(hk_scene_builder* b, uint32_t mesh_id);
/* The host twin of hk_rebuild_mesh_tree (HK_TREE_SAH): the mesh's tree built again over its CURRENT triangles, as
 * hk_scene_builder_add_mesh would build it for these positions (`bvh` 0.7.1 BVH::build), every navigator box then the union of the two
 * boxes below it as hk_scene_builder_set_mesh_vertices forms them.  Primitives, vertices and the mesh box are untouched; the node
 * count stays (3n - 2).  An error leaves the builder as it was.  The next finish lays the mesh level out again. */
int hk_scene_builder_rebuild_mesh_tree(hk_scene_builder* b, uint32_t mesh_id);
/* A mesh whose tree is DEFERRED: hk_scene_builder_add_mesh with the same arguments, validation, primitives, vertices and mesh box, but
 * without its `BVH::build` - the mesh gets a valid stand-in tree of the final size (3n - 2 nodes, flatten_custom layout, the index list
 * halved recursively) and is marked pending.  Offsets and HkMeshIndex records are final at the next finish (the node count does not
 * depend on the tree).  hk_load_scene builds the pending trees on the device; hk_scene_builder_build_pending_mesh_trees is the host
 * completion (per pending mesh the tree of hk_scene_builder_rebuild_mesh_tree, written in place: a finished builder stays finished and
 * its getters return the final trees).  Every other upload of a builder with pending meshes is refused (HK_E_NOT_READY). */
int hk_scene_builder_add_mesh_deferred(hk_scene_builder* b, const float* positions, const float* normals, const float* uvs,
                                       uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, uint32_t topology,
                                       uint32_t* mesh_id);
int hk_scene_builder_pending_mesh_trees(const hk_scene_builder* b, uint32_t* count);
int hk_scene_builder_build_pending_mesh_trees(hk_scene_builder* b);
/* A mesh DECLARED by its counts: its arrays are still to come - from device memory (hk_add_meshes_device) or, the host twin and the
 * fallback, from hk_scene_builder_resolve_mesh.  n_indices == 0 is the identity list over the vertices (mod.rs:408-411); the triangle
 * count is the one hk_scene_builder_add_mesh arrives at (a list n / 3, a strip n - 2).  The mesh holds n_vertices zero vertices, that
 * many zero primitives and the deferred mesh's stand-in tree of the final 3t - 2 nodes, and carries two marks: pending (its tree is a
 * stand-in) and UNRESOLVED (its geometry is zeros).  The next finish gives it its final HkMeshIndex - the record a twin that used
 * hk_scene_builder_add_mesh_deferred gets.  Validation is add_mesh's where it applies: n_vertices == 0 or no triangle HK_E_INVALID; an
 * unknown topology, or a list whose count is no multiple of 3, HK_E_UNSUPPORTED; the builder is unchanged then.
 * While a mesh is unresolved: hk_scene_builder_add_instance naming it returns HK_E_NOT_READY (its box is unknown: instances follow the
 * add, the documented flow of hk_add_meshes); hk_upload_scene, hk_load_scene, hk_add_meshes, hk_scene_builder_build_pending_mesh_trees
 * (and the hk_multi_ forms), as well as the mesh edits of the builder that name it, return HK_E_NOT_READY naming the mesh, with nothing
 * written; hk_scene_builder_remove_mesh works and takes both marks along.
 * hk_scene_builder_resolve_mesh fills a declared mesh from HOST arrays with add_mesh's own arithmetic (positions, normals: 3 floats per
 * vertex; uvs: 2, or NULL = (0, 0); indices: the declared count, NULL iff it was declared with none): vertices, primitives (a strip's
 * odd triangles flipped), the mesh box as Aabb::from_min_max over ALL vertices, the stand-in over the real triangle boxes.  In a finished
 * builder the concatenated arrays are patched in place and the builder stays finished.  The mesh then is an ordinary deferred mesh.
 * HK_E_INVALID with the builder unchanged: NULL, a mesh that is not unresolved, indices given or missing against the declaration, an
 * index >= n_vertices.  hk_scene_builder_unresolved_meshes counts the meshes that still wait. */
int hk_scene_builder_declare_mesh(hk_scene_builder* b, uint32_t n_vertices, uint32_t n_indices, uint32_t topology, uint32_t* mesh_id);
int hk_scene_builder_resolve_mesh(hk_scene_builder* b, uint32_t mesh_id, const float* positions, const float* normals, const float* uvs,
                                  const uint32_t* indices);
int hk_scene_builder_unresolved_meshes(const hk_scene_builder* b, uint32_t* count);
/* the HkMeshIndex of a mesh after a finish (what its instances carry, and what the hk_*_mesh_* calls take) */
int hk_scene_builder_mesh_index(const hk_scene_builder* b, uint32_t mesh_id, HkMeshIndex* out);
/* Meshes that leave (the twin of hk_scene_builder_remove_instance).  hk_scene_builder_mesh_extent: the mesh's ranges in the arrays of the
 * last finish - also the layout of a context that has taken all of the builder's meshes; node_count 0 for a mesh no finish has seen.
 * hk_scene_builder_remove_mesh: the ids of the meshes added after the removed one shift down by one, the mesh ids of the instance
 * declarations with them; a deferred mesh takes its mark along.  The mesh level is un-finished: the next finish concatenates again from
 * the removed mesh on, what lies in front of it keeps its bytes, and the builder then holds, getter for getter, what a builder that never
 * had the mesh holds.  `removed` (or NULL) receives the extent in the coordinates of the last finish - they stay in those coordinates
 * for every removal until the next finish, which is what hk_remove_meshes takes in one call.  HK_E_INVALID with the builder unchanged
 * (still finished if it was) for NULL, an unknown id, and a mesh an instance declaration still names. */
int hk_scene_builder_mesh_extent(const hk_scene_builder* b, uint32_t mesh_id, HkMeshExtent* out);
int hk_scene_builder_remove_mesh(hk_scene_builder* b, uint32_t mesh_id, HkMeshExtent* removed);
/* Pure host logic, no context: the record `index` as it reads once removed[0..n) are gone - each of vertex, primitive and node_offset
 * minus the number of removed elements in front of it (an extent that surrounds the value counts up to the value); node_count is kept. */
int hk_rebase_mesh_index(const HkMeshExtent* removed, uint32_t n, const HkMeshIndex* index, HkMeshIndex* out);

/* The layout conversion behind HK_CTX_EXACT_TRAVERSAL's opposite (see there): `nodes[0..count)` is ONE flat BVH in the `bvh`
 * 0.7.1 flatten_custom layout the reference produces (mod.rs:185-201,458-459; entry / exit indices local to the array);
 * `out` receives the same tree flattened for ray-direction octant `octant` (bit k set = direction component k negative).
 * Pure host logic. */
int hk_bvh_rethread(const HkNode* nodes, uint32_t count, uint32_t octant, HkNode* out);

/* ------------------------------------------------------------------ uploads (Prepare stage) */
/* MeshRenderAssets::set + write_buffer, mesh.rs:43-64 (3 global buffers) */
int hk_upload_meshes(hk_ctx* ctx, const HkVertex* vertices, uint32_t n_vertices, const HkPrimitive* primitives,
                     uint32_t n_primitives, const HkNode* asset_nodes, uint32_t n_asset_nodes);
/* MaterialRenderAssets, material.rs:201-202.  The *_texture fields index the array given to
 * hk_upload_textures (HK_NO_TEXTURE = none), exactly like MaterialTextures::id (material.rs:76-86). */
int hk_upload_materials(hk_ctx* ctx, const HkMaterial* materials, uint32_t n_materials);
/* The `textures` / `samplers` binding arrays of group 3 (light.wgsl:15-18, mod.rs:760-782): one
 * RGBA8 image + its sampler per entry, sampled at LOD 0 (light.wgsl:749-793).  is_srgb = the image
 * format is Rgba8UnormSrgb (bevy loads base-colour / emissive images that way): rgb is decoded to
 * linear BEFORE filtering, alpha is linear.  n = 0 selects the NO_TEXTURE pipelines. */
typedef enum HkAddressMode { HK_ADDRESS_CLAMP_TO_EDGE = 0, HK_ADDRESS_REPEAT = 1, HK_ADDRESS_MIRROR_REPEAT = 2 } HkAddressMode;
typedef struct HkImageDesc {
  const uint8_t* rgba8; /* width * height * 4 bytes, row-major, row 0 = v = 0 */
  uint32_t width, height;
  uint32_t is_srgb;
  uint32_t address_u, address_v; /* HkAddressMode */
  uint32_t filter_linear;        /* 0 = nearest, 1 = bilinear (mag/min filter of the image's sampler) */
} HkImageDesc;
/* Instance motion on the DEVICE.  The reference re-runs prepare_instances on the CPU whenever an instance
 * moves (instance.rs:286-437): per-instance world AABB and inverse-transpose matrix, the emitter records that follow from them
 * (position, radius, surface area, alias table), a fresh `BVH::build` of the instance tree and of the light tree, and a re-upload
 * of all five buffers.  hk_upload_scene_instances is that path (host rebuild, asynchronous upload into the spare slot).  This
 * entry point instead diffs the builder's poses (hk_scene_builder_set_instance_transform) against the poses the device holds and
 * hands the moved instances - 96 B each, read by the kernel from pinned memory - to the GPU: one kernel redoes the per-instance and
 * per-emitter work with the host builder's exact arithmetic, two more REFIT the instance tree (in all of its direction-threaded
 * orderings) and the light tree: same topology, every inner box the union of the leaf boxes below it.  Stream-ordered, no host or
 * device wait; frames in flight keep the slot they were enqueued with.  What it does NOT do is change the shape of the trees: after
 * large displacements a host calls hk_rebuild_scene_trees (below) now and then to get the reference's SAH tree back (any-hit
 * identity and tie-breaks follow the tree, so a refit frame equals the reference frame for THAT tree, not for the rebuilt one).
 * Instances must be the ones uploaded (same count, meshes, materials); *moved (optional) = how many poses changed.  The builder's
 * previous-transform bookkeeping advances as it would in hk_scene_builder_finish.
 * After a device-side update the host copies of the trees and emitter records are stale: an upload that re-lays the instance-level
 * region out from them (hk_upload_materials, hk_upload_textures) is refused with HK_E_NOT_READY at the next frame until
 * hk_upload_scene_instances / hk_upload_instances brings the host's version of the scene back.
 * After an hk_update_materials that switched an emitter (its case B took the builder's poses along) a refit called before the next
 * frame with no pose left to change returns at once: the instances that moved in that update keep their `moved` flag for the frame. */
int hk_refit_scene_instances(hk_ctx* ctx, hk_scene_builder* b, uint32_t* moved);
/* ... and the REBUILD on the device, for when refits have degraded a tree: new trees over the instances' and the emitters' current
 * boxes, written in place in the flatten_custom layout (all direction-threaded orderings of the instance tree; child order of
 * orderings 1-7 by the rule of hk_bvh_rethread).
 *   HK_TREE_SAH   the reference's OWN tree: `bvh` 0.7.1's binned-SAH build (BVH::build, instance.rs:365-371,422-428) level by level in
 *                 one workgroup - every reduction in it is a min, a max or a count and its re-ordering a stable sort by bucket, so
 *                 the parallel build makes the host's decisions and returns the host's tree shape (the tests compare the links).
 *                 A frame after it equals the frame after hk_upload_scene_instances.
 *   HK_TREE_LBVH  Morton codes of the box centres, one radix sort, Karras' parallel hierarchy: a few kernels whatever the depth of
 *                 the tree, but spatial-median splits - a worse tree (frames 17-23 % slower in the probe scenes); frames equal the
 *                 reference's up to exact ties between candidates, like any other valid tree over the same instances. */
#define HK_TREE_SAH 0u
#define HK_TREE_LBVH 1u
/* Instances ADDED, REMOVED or given another material (hk_scene_builder_add_instance / _remove_instance /
 * _set_instance_material, any number of pose changes with them): hk_scene_builder_finish_instances lays the instance-level
 * records out on the host (O(instances); no tree build), the asynchronous upload puts them into the spare slot and both trees
 * are built on the device in `tree_mode` - with HK_TREE_SAH the result is what hk_scene_builder_finish +
 * hk_upload_scene_instances gives (the reference's path), minus the two host-side SAH builds that dominate it.
 * Materials APPENDED on the builder since the context took its materials travel with the call (a spawned object is a mesh - hk_add_meshes -
 * a material and an instance); a texture id at or above the uploaded texture count is refused (HK_E_INVALID), as hk_update_materials
 * refuses it.  Changed values of existing materials keep going through hk_update_materials.
 * Refused with HK_E_NOT_READY once a mesh was deformed on the device or the poses came from device memory: the mirrors it lays out from
 * are stale then.  hk_change_scene_instances (below) is the way on in those states. */
int hk_update_scene_instances(hk_ctx* ctx, hk_scene_builder* b, uint32_t tree_mode);
int hk_rebuild_scene_trees(hk_ctx* ctx, uint32_t mode);
/* The instance set changed, in EVERY state of the scene: after mesh deformations (hk_update_mesh_vertices, hk_skin_mesh, hk_deform_meshes*)
 * and after poses set from device memory (hk_set_instance_transforms_device) too, where hk_update_scene_instances is refused because the
 * host's copies of boxes, triangle areas and poses are stale.  The LAYOUT of the instance level never is - counts, offsets, which instance
 * emits, the length of every alias slice follow from topology and materials - so the host lays the new level out as ever into the spare
 * slot and the device writes its own values over the stale ones, in stream order, with no host wait on a warm call:
 *   `b` is the scene's builder after any number of hk_scene_builder_add_instance / _remove_instance / _set_instance_material calls (mesh
 * additions and removals have gone through hk_add_meshes / hk_remove_meshes first); n is its instance count; origins[k] is the id
 * instance k had in the scene the context holds, or HK_INSTANCE_NEW - the builder shifts ids on removal, so the caller states the map.
 * Materials appended on the builder travel with the call, as in hk_update_scene_instances.
 *   - layout, mesh and material words: the host's (hk_scene_builder_finish_instances).  A survivor is an instance of its origin's mesh.
 *   - a new instance takes the builder's pose and enters at rest.
 *   - a survivor, poses on the device: keeps the model and inverses the device holds (the builder's transform for it is ignored, as
 *     hk_set_instance_transforms_device ignores it for unnamed instances) and is at rest.  Poses not on the device: the builder's pose,
 *     at motion if it differs from the previous one, and the builder's previous-transform bookkeeping advances - hk_update_scene_instances.
 *   - world boxes: the mesh's current box - the device's for a deformed mesh, the builder's otherwise - through the instance's model.
 *   - emitter records, surface areas and alias slices: from those boxes and the triangles the device holds.
 *   - both trees: built on the device in `tree_mode`, as hk_rebuild_scene_trees builds them; a tree of one leaf is the host's.
 * With HK_TREE_SAH the instance level ends what a fresh hk_upload_scene of the same meshes (current vertices and tree shapes), poses,
 * instance set and materials leaves.  Where hk_update_scene_instances is accepted the call takes that call's path and leaves its bytes.
 * When the spare slot has no room the scene moves once, device to device in one launch, to slots half again the need; frames in flight
 * keep the allocation they were enqueued with (freed once they are past it).  Deformations, device poses, refits and material edits
 * issued afterwards land on the new ids.  Whether meshes are deformed and whether the poses are the device's stays as it was.
 * Refused with nothing written: HK_E_INVALID for NULL arguments, an unknown tree_mode, n other than the builder's instance count, an
 * origin out of range or named twice, a survivor of another mesh than its origin's, a singular or non-finite pose of a new instance (of
 * any instance while the poses are the host's), a texture id at or above the uploaded count; HK_E_NOT_READY without a scene, for a
 * builder with unfinished mesh changes or deferred meshes, for a scene walked from its LDS copy (one slot) whose mirrors are stale or
 * whose meshes are deformed (the rule of hk_add_meshes / hk_remove_meshes), and - in the stale states - for an instance of a mesh that no
 * instance had used when the mesh level was last laid out on the host (its tree has no leaf boxes; meshes from hk_add_meshes have them). */
#define HK_INSTANCE_NEW 0xFFFFFFFFu
int hk_change_scene_instances(hk_ctx* ctx, hk_scene_builder* b, const uint32_t* origins, uint32_t n, uint32_t tree_mode);
/* Material edits on the DEVICE.  The builder's materials (hk_scene_builder_set_material; the builder need not be finished) are diffed
 * against the materials the context holds, as hk_refit_scene_instances diffs poses; *changed (optional) = the records that differ.
 * With none the call returns HK_OK and enqueues nothing.  Otherwise one of two cases, decided inside the call by the builder's own rule
 * for which instances emit (255 a |rgb| of the material's emissive colour > 0, instance.rs:380-382):
 *   A  the set of emitting instances stays.  Everything happens on the device, stream-ordered like a refit: no host wait, in the spare
 *      slot of a two-slot scene and in place behind everything enqueued in a one-slot scene, after the boxes of meshes deformed since
 *      the last frame have reached the instance level.  The changed records (80 B each) are read by a kernel from pinned,
 *      double-buffered memory and written into the slot's material array.  Only if a changed material's emissive colour differs bit for
 *      bit, one more kernel re-derives position and radius (0.5 |max - min| + sqrt(255 a |rgb|), instance.rs:382,409) of every emitter
 *      whose instance uses such a material, from the instance's CURRENT device box, and the light tree is refit in its current shape -
 *      the rule of hk_refit_scene_instances; hk_rebuild_scene_trees brings the SAH shape back.  The instance tree, its wide records, the
 *      alias tables and surface areas are untouched; `tree_mode` is validated and not used; the builder's previous-transform
 *      bookkeeping does not advance.  The host copies become stale (see hk_refit_scene_instances) only if an emitter record changed:
 *      an edit of base colours on a context never refit leaves hk_upload_textures and the other relayout paths usable.  Case A works
 *      after refits, device tree rebuilds and mesh deformations - the states in which hk_upload_materials is refused.
 *   B  an emitter is switched on or off: the emitter list, the alias tables and the light tree change size.  The context takes the new
 *      materials and does what hk_update_scene_instances(ctx, b, tree_mode) does - hk_scene_builder_finish_instances, the asynchronous
 *      upload into the spare slot, both trees built on the device - with that call's contract: HK_TREE_SAH gives the host builder's
 *      trees link for link, HK_E_NOT_READY after a mesh deformation, poses set on the builder since the last update are taken along and
 *      the transform bookkeeping advances.  A builder whose instance set is not the uploaded one (instances added or removed, another
 *      mesh or material for one - what hk_refit_scene_instances refuses) takes this path too whenever a material record changed, so
 *      the pending edit travels with it; with no record changed the call enqueues nothing and such edits wait for
 *      hk_update_scene_instances.
 * So in a frame that both moves instances and edits materials, call hk_update_materials BEFORE hk_refit_scene_instances: the refit then
 * finds nothing left to do in case B and does the motion in case A.
 * Refused with nothing written: NULL, an unknown tree_mode, a builder whose material count differs from the uploaded one (materials
 * added go through hk_upload_scene), a changed record naming a texture id >= the uploaded texture count (HK_E_INVALID); no scene, a
 * builder with unfinished mesh changes or deferred meshes (HK_E_NOT_READY). */
int hk_update_materials(hk_ctx* ctx, hk_scene_builder* b, uint32_t tree_mode, uint32_t* changed);
/* Mesh deformation on the DEVICE: new vertex data for one uploaded mesh, its BLAS refit in every layout that holds it, the change
 * carried up to the instances of the mesh (world AABBs, emitter records and alias tables) and to the instance tree and the light tree.
 * A mesh is named by the HkMeshIndex its instances carry (it must equal an uploaded instance's record); its topology (index buffer,
 * triangles, uvs, tree links) never changes, only positions and normals do.  Stream-ordered like
 * hk_refit_scene_instances: host data goes through pinned staging, frames enqueued before the call see the old mesh and frames enqueued
 * after it the new one; there is no host wait (pinned staging from a pool, reused once the device has read it).  The mesh level is
 * written at the call; the instances, emitters and both instance-level trees follow once, before whatever reads them next (the next
 * frame), for all meshes deformed in between.  `n_vertices` must be exactly the vertices the mesh's triangles span (highest index + 1).
 * Argument errors return HK_E_INVALID with nothing written.
 * After a deformation the host copies of the mesh (vertices, BLAS boxes, the mesh box behind the instance boxes) are stale: what would
 * lay scene memory out again from them is refused with HK_E_NOT_READY until hk_upload_scene brings the host's mirror of the change
 * (hk_scene_builder_set_mesh_vertices) back - hk_upload_instances / hk_upload_scene_instances / hk_update_scene_instances at the call,
 * hk_upload_materials / hk_upload_textures at the next frame (as after hk_refit_scene_instances); hk_rebuild_scene_trees and
 * hk_refit_scene_instances work from the device's current boxes.  A scene walked through its one-level
 * tree (HK_TRAVERSAL_ONE_LEVEL) walks its two-level trees from the first deformation until that upload (hk_traversal_mode reports it).
 * hk_upload_meshes (and so hk_upload_scene) drops every skin set below. */
/* positions: n_vertices x 3 floats; normals: n_vertices x 3 floats or NULL (keep the current ones) */
int hk_update_mesh_vertices(hk_ctx* ctx, const HkMeshIndex* mesh, uint32_t n_vertices, const float* positions, const float* normals);
/* Linear-blend skinning (Bevy 0.9 skinning.wgsl), set once per mesh: bind-pose positions and normals (n_vertices x 3 floats), up to
 * four joints per vertex (n_vertices x 4 uint16, Bevy's JOINT_INDEX) and their weights (n_vertices x 4 floats, JOINT_WEIGHT; used as
 * given, not renormalised). */
int hk_set_mesh_skin(hk_ctx* ctx, const HkMeshIndex* mesh, uint32_t n_vertices, const float* bind_positions, const float* bind_normals,
                     const uint16_t* joint_indices, const float* joint_weights);
/* per frame: n_joints column-major 4x4 joint matrices; the device skins the mesh (positions and normals, mesh-local) and refits as
 * hk_update_mesh_vertices does.  A joint index >= n_joints in the skin is refused (HK_E_INVALID, nothing written). */
int hk_skin_mesh(hk_ctx* ctx, const HkMeshIndex* mesh, const float* joint_matrices, uint32_t n_joints);
/* MANY meshes deformed in one call: item k is what hk_update_mesh_vertices (HK_DEFORM_VERTICES) or hk_skin_mesh (HK_DEFORM_SKIN) takes for
 * one mesh.  After the call the context is in every respect what the n single-mesh calls in item order would have left - device bytes,
 * what is stale, what is refused afterwards - but the device work is a fixed number of kernel launches, however many items there are
 * (a crowd of skinned characters costs what one character costs to enqueue), and so is what follows before the next frame: the new
 * boxes reach the instances and emitters of all deformed meshes in one launch each, the wide records of their trees are derived in
 * one.  Composes with hk_refit_scene_instances, hk_rebuild_mesh_tree, the single-mesh calls and frames in flight as those calls do.
 * The whole batch is validated before anything is enqueued or written: the first bad item returns its error with the item's index
 * in hk_last_error(), the scene untouched.  Per item the checks of the single calls (unknown mesh record, vertex count out of range,
 * no skin set, a joint index >= count, NULL data, normals on a skin item, unknown kind: HK_E_INVALID); a mesh named twice in one
 * batch is HK_E_INVALID.  n == 0 returns HK_OK and does nothing.  Once every mesh of the batch has been deformed before and nothing
 * has to grow, the call neither waits for the device nor allocates: the item table, every item's data and the joint palettes travel
 * in ONE pinned staging block from the pool. */
#define HK_DEFORM_VERTICES 0u   /* what hk_update_mesh_vertices takes */
#define HK_DEFORM_SKIN     1u   /* what hk_skin_mesh takes; hk_set_mesh_skin must have been called for the mesh */
typedef struct HkMeshDeform {
  HkMeshIndex  mesh;
  uint32_t     kind;
  uint32_t     count;    /* VERTICES: n_vertices.  SKIN, MORPH_SKIN: n_joints.  MORPH: n_targets */
  const float* data;     /* VERTICES: count x 3 positions.  SKIN, MORPH_SKIN: count x 16 joint matrices, column-major.  MORPH: count weights */
  const float* normals;  /* VERTICES: count x 3, or NULL = keep.  SKIN, MORPH: must be NULL.  MORPH_SKIN: the set's n_targets weights */
} HkMeshDeform;
int hk_deform_meshes(hk_ctx* ctx, const HkMeshDeform* items, uint32_t n);
/* ... and the same batch with its SOURCES IN DEVICE MEMORY (a cloth solver's positions, a joint palette animated on the GPU): the call
 * leaves the context in every respect as hk_deform_meshes leaves it when given the same values from host memory - device bytes, what
 * is stale, what is refused afterwards, how it composes with refits, rebuilds, hk_add_meshes and frames in flight.  Only the item
 * table travels through pinned staging; positions, normals and palettes are read where they lie, so a stride names a column slice of a
 * larger state tensor ([n, 8], say) without a copy.  Positions and normals need 4-byte alignment, palettes 16-byte alignment.
 *   Ordering.  With producer_stream (a hipStream_t) != NULL the context's stream waits for an event recorded on that stream at the
 * call, before its first launch, and the producer stream then waits for an event recorded behind the last kernel that reads the
 * sources (the vertex kernel; palettes are copied to the mesh's own memory before it): the caller may overwrite its buffers in stream
 * order right after the call returns.  No host wait.  With NULL the caller has ordered itself (the rule of hk_cast_rays_device).
 *   Validation.  Every check of hk_deform_meshes, and HK_E_INVALID for: a source pointer that is neither memory of the context's
 * device nor host memory the device can access (plain pageable memory is refused: a mistaken pointer cannot fault the device) or whose
 * extent leaves its allocation, a misaligned pointer, a bad stride, an unknown flag bit, HK_DEFORM_RECOMPUTE_NORMALS on a skin item or
 * together with normals.  The whole batch is validated before anything is enqueued.
 *   HK_DEFORM_RECOMPUTE_NORMALS (VERTICES items): after the item's positions have landed its vertex normals are recomputed, all in f32
 * in the stated order, without contraction.  The face vector of triangle t with corners p0, p1, p2 (the order of HkPrimitive.vertices),
 * e1 = p1 - p0, e2 = p2 - p0, is f = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x), un-normalised (the sum is
 * area-weighted).  The normal of vertex v is s = ((+0 + f[t_1]) + f[t_2]) + ... per component over the corners that name v, in
 * ascending triangle index and then corner index; (s.x, s.y, s.z, 0) is stored un-normalised as every other path stores normals.  If
 * all three components of s compare equal to zero (a vertex no triangle names included) the vertex keeps its current normal.  The
 * result does not depend on scheduling (a gather over a per-mesh corner list, built on the mesh's first such call - one wait there).
 * hk_scene_builder_recompute_mesh_normals is the host twin.  A batch with a flagged item is six launches, five otherwise. */
#define HK_DEFORM_RECOMPUTE_NORMALS 1u
typedef struct HkMeshDeformDevice {
  HkMeshIndex mesh;
  uint32_t    kind;            /* HK_DEFORM_VERTICES / HK_DEFORM_SKIN / HK_DEFORM_MORPH / HK_DEFORM_MORPH_SKIN */
  uint32_t    count;           /* VERTICES: n_vertices.  SKIN, MORPH_SKIN: n_joints.  MORPH: n_targets */
  const void* data;            /* DEVICE memory.  VERTICES: positions, 3 floats per vertex at data + v * data_stride.  SKIN, MORPH_SKIN: count x 16 floats, column-major, contiguous.  MORPH: count weights, contiguous */
  const void* normals;         /* DEVICE memory, 3 floats per vertex at normals + v * normals_stride, or NULL.  MORPH_SKIN: the set's n_targets weights, contiguous */
  uint32_t    data_stride;     /* bytes; 0 = packed (12).  VERTICES only: >= 12, a multiple of 4.  SKIN, MORPH_SKIN: 0 or 64.  MORPH: 0 or 4 */
  uint32_t    normals_stride;  /* bytes; 0 = packed (12).  MORPH_SKIN: 0 or 4 */
  uint32_t    flags;           /* HK_DEFORM_RECOMPUTE_NORMALS */
  uint32_t    _pad;
} HkMeshDeformDevice;          /* 56 bytes */
int hk_deform_meshes_device(hk_ctx* ctx, const HkMeshDeformDevice* items, uint32_t n, void* producer_stream);
/* MORPH TARGETS (blend shapes, glTF 2.0 section 3.7.2.2) blended on the device, as items of the two batch calls above.  A morph set is
 * given once per mesh, like a skin: base positions and normals (n_vertices x 3 floats each) and n_targets dense targets, target-major -
 * delta k of vertex v at [(k * n_vertices + v) * 3] of position_deltas and of normal_deltas (or NULL: the normals do not morph).  Per
 * frame an item carries only the n_targets weights; the deltas never cross the bus again.
 *   HK_DEFORM_MORPH       count = the set's n_targets, data = count weights (floats), normals must be NULL
 *   HK_DEFORM_MORPH_SKIN  count = n_joints, data = the palette as for HK_DEFORM_SKIN; `normals` names the set's n_targets weights.  The
 *                         morphed position and normal of a vertex take the place of the skin's bind position and normal in the skinning
 *                         arithmetic of hk_skin_mesh (in registers: nothing is written in between); palette, joint indices and joint
 *                         weights are those of hk_set_mesh_skin, whose bind planes are not read.  Needs a morph set and a skin of the
 *                         same vertex count.
 *   The numeric contract.  All in f32, no contraction: each product is rounded, then each sum.  Per component
 *     p = ((base + w[a1] * dp[a1]) + w[a2] * dp[a2]) + ...
 * over the ACTIVE targets a1 < a2 < ... in ascending target index.  A target is active iff its weight does not compare equal to zero:
 * +0 and -0 are skipped, a NaN weight is active.  A skipped target contributes nothing - no signed zero, no NaN from an infinite delta.
 * Normals follow the same rule with the normal deltas; without normal deltas every call writes the base normals.  Normals are stored
 * un-normalised, as on every other path.  Weights are used as given, neither clamped nor normalised.  hk_morph_vertices is the host
 * twin of this arithmetic (no context, no GPU).
 *   After a MORPH item the context is in every respect what a HK_DEFORM_VERTICES item carrying hk_morph_vertices' positions and normals
 * would have left; after a MORPH_SKIN item what hk_set_mesh_skin(the morphed bind pose) followed by a HK_DEFORM_SKIN item would have
 * left - device bytes, what is stale, what is refused afterwards, how it composes with refits, rebuilds and frames in flight.  A batch
 * with morph items stays at five launches and one pinned staging block, and does not wait for the device once nothing has to grow.
 *   State.  A set replaces an earlier one behind a wait for the device, as a skin does; hk_upload_meshes / hk_upload_scene drop morph
 * sets as they drop skins; hk_add_meshes, refits and rebuilds leave them alone.  n_vertices must be the mesh's vertex count.
 *   Validation (the whole batch before anything is enqueued, item index in hk_last_error(); HK_E_INVALID): no morph set for the mesh;
 * MORPH with count != the set's target count or with normals != NULL; MORPH_SKIN with normals == NULL, without a skin or with a skin
 * of another vertex count, or a joint index >= count; HK_DEFORM_RECOMPUTE_NORMALS on either kind.  hk_deform_meshes_device: weights
 * are a source like any other (4-byte alignment, n_targets x 4 bytes inside their allocation), data_stride of a MORPH item and
 * normals_stride of a MORPH_SKIN item must be 0 or 4.  The set call: n_targets == 0 or > HK_MORPH_MAX_TARGETS, a NULL pointer (but
 * normal_deltas) or a vertex count that is not the mesh's is HK_E_INVALID, a failed allocation HK_E_NOMEM. */
#define HK_DEFORM_MORPH      2u
#define HK_DEFORM_MORPH_SKIN 3u
#define HK_MORPH_MAX_TARGETS 4096u
int hk_set_mesh_morph_targets(hk_ctx* ctx, const HkMeshIndex* mesh, uint32_t n_vertices, uint32_t n_targets, const float* base_positions,
                              const float* base_normals, const float* position_deltas, const float* normal_deltas);
/* the vertex arithmetic above on the host: positions_out and normals_out (n_vertices x 3 floats each) from the arrays of a set and
 * n_targets weights.  HK_E_INVALID for a NULL pointer (but normal_deltas), n_vertices == 0, n_targets == 0 or > HK_MORPH_MAX_TARGETS. */
int hk_morph_vertices(uint32_t n_vertices, uint32_t n_targets, const float* base_positions, const float* base_normals,
                      const float* position_deltas, const float* normal_deltas, const float* weights, float* positions_out,
                      float* normals_out);
/* Instance POSES FROM DEVICE MEMORY (rigid bodies stepped on the GPU, a crowd placed by a kernel): what hk_refit_scene_instances does for
 * poses the host never sees.  After the call the device scene holds, byte for byte, what hk_refit_scene_instances would have left had the
 * same values been set on the builder with hk_scene_builder_set_instance_transform: instance records, previous models, world boxes,
 * emitter records with their alias tables, both trees refit in their shape; the same statistics (scene_device_refits += 1).
 *   instance_ids (HOST memory) names n distinct instances, pose k at d_models + k * stride_bytes (16 floats, column-major; stride_bytes
 * >= 64 and a multiple of 4; 4-byte alignment is all a pose needs).  NULL names instances 0 .. n - 1.
 *   Which instance moved is decided on the device.  A named instance whose 16 floats equal the model the device holds bit for bit is at
 * rest (`moved` cleared, previous model = model); any other named instance takes the pose and keeps the model it had as its previous
 * one; an instance the call does not name is at rest, whichever call moved it last (a pass over all instances clears the flags first).
 *   A pose that is not finite or has no inverse (the builder's own test: the determinant of the double-precision cofactor expansion is
 * 0) is not taken: the instance keeps its pose and is at rest.  d_status (DEVICE memory, 4 bytes, or NULL) receives 1 + the highest
 * such instance id of the call, or 0, in stream order - the call cannot return an error for values it has not read.
 *   `b` is the builder the scene came from: it supplies each instance's mesh box (kept in a device plane and copied only when it changed:
 * a warm call copies nothing per instance beyond the 8 bytes of a named id) and is validated as hk_refit_scene_instances validates it
 * (same instance count, meshes, materials; finished mesh level).  Its previous-transform bookkeeping does not advance: it was not told.
 * Meshes deformed on the device keep their device box, as after hk_refit_scene_instances.
 *   Ordering: the rule of hk_deform_meshes_device.  With producer_stream != NULL the context's stream waits for an event recorded there
 * at the call, and the producer then waits for an event behind the kernel that reads d_models (and writes d_status): the caller may
 * overwrite the poses in stream order right after the call.  NULL: the caller has ordered itself.  A warm call - not the first for an
 * instance list - never waits on the host; two-slot scenes are updated in the spare slot, one-slot scenes in place behind everything
 * enqueued.
 *   Validated as a whole before anything is enqueued; HK_E_INVALID with nothing written for: NULL ctx / b / d_models, ids given with n ==
 * 0, n or an id beyond the instance count, an id named twice, a bad stride, d_models or d_status misaligned (4 bytes), not memory of the
 * context's device nor host memory mapped for it, or reaching beyond its allocation; a builder that is not the scene's.  HK_E_NOT_READY
 * without a scene or for a builder with unfinished mesh changes.
 *   Afterwards the host's copies of the poses, boxes and previous models no longer describe the device (as its trees and emitter records
 * do not after any device-side update).  What would diff against or lay out from them is refused with HK_E_NOT_READY:
 * hk_refit_scene_instances, hk_update_scene_instances, case B of hk_update_materials, hk_scene_bounds; a band of a sharded frame that
 * derives its history rows takes all of them.  The one-level walk and the shared-transform shortcut are off (hk_traversal_mode reports
 * it).  Case A of hk_update_materials, hk_rebuild_scene_trees, hk_add_meshes, the deformation calls, hk_rebuild_mesh_tree, hk_cast_rays*
 * and hk_update_texture work from device state and stay usable.  hk_upload_scene_instances / hk_upload_instances / hk_upload_scene end
 * the state.  Instances are added, removed and re-materialed in it through hk_change_scene_instances, which keeps the device's poses.
 * There is no hk_multi_ form, as hk_deform_meshes_device has none: a device pointer lives on one device. */
int hk_set_instance_transforms_device(hk_ctx* ctx, hk_scene_builder* b, const uint32_t* instance_ids, uint32_t n, const void* d_models,
                                      uint32_t stride_bytes, void* producer_stream, uint32_t* d_status);
/* ... and the way back: waits for the context's streams and copies the models the device holds - the slot the next frame would read - to
 * `models` (n x 16 floats, n = the instance count).  The context's own copies of the models follow; the state above stays until the host
 * has put the poses on its builder and called hk_upload_scene_instances. */
int hk_read_instance_transforms(hk_ctx* ctx, float* models, uint32_t n);
/* ... and the REBUILD of one mesh's tree on the device, for when refits have degraded it (a skinned character far from its bind pose,
 * a cloth folded onto itself): a new tree over the mesh's current triangle boxes, written in place over the mesh's nodes in the
 * mesh-level region - ordering 0 in the builder's left-before-right order, orderings 1-7 by the rule of hk_bvh_rethread, single-leaf
 * navigators folded - and the topology the refit climbs replaced by the new tree's, so that the next hk_update_mesh_vertices /
 * hk_skin_mesh refits the NEW shape.  Skins stay.  The mesh box and the triangle order do not change: nothing at the instance level moves.
 *   HK_TREE_SAH   the tree hk_scene_builder_rebuild_mesh_tree builds, node for node and byte for byte.  Meshes above 32 768 triangles
 *                 run the top levels of the build on the whole chip (a fixed number of multi-workgroup levels, the rest one workgroup
 *                 per subtree); smaller ones in one workgroup as the instance tree does.
 *   HK_TREE_LBVH  the Morton build: a valid tree, not the host's.
 * Contract of a deformation (see above): stream-ordered behind everything enqueued, no host wait except a rare growth of the build
 * scratch (about 330 B per triangle, kept in the context); the host mirrors are stale afterwards - re-layouts are refused with
 * HK_E_NOT_READY and the one-level walk is off until hk_upload_scene brings the builder's twin.  A mesh never deformed works too.
 * Refused with nothing written: an unknown mesh record or mode (HK_E_INVALID), no scene (HK_E_NOT_READY), a mesh of more than
 * HK_MESH_REBUILD_MAX_TRIANGLES triangles (HK_E_UNSUPPORTED). */
#define HK_MESH_REBUILD_MAX_TRIANGLES 4194304u
int hk_rebuild_mesh_tree(hk_ctx* ctx, const HkMeshIndex* mesh, uint32_t mode);
/* Motion vectors for one deforming mesh, on (enable != 0) or off.  By default velocity_uv.xy is the reference's formula: the previous
 * INSTANCE transform applied to the CURRENT hit point, so a deformation counts as no motion and everything that reprojects through
 * the plane (the temporal light passes, the spatial pass's history, SMAA Tu4x, TAA) fetches another surface point's history on a
 * skinned or morphed mesh.  An enabled mesh keeps its PREVIOUS local positions on the device (one float4 per vertex, +16 B per vertex):
 * the previous positions of frame k are the positions the mesh had when frame k - 1's primary rays were enqueued.  A pixel whose closest
 * hit lies on such a mesh deformed since then gets
 *   velocity = clip_to_uv(view_proj * world) - clip_to_uv(previous_view_proj * M_prev * (P0 + b.x (P1 - P0) + b.y (P2 - P0), 1))
 * with P0..P2 the previous positions of the hit triangle's corners, b the hit's barycentrics and M_prev the instance's previous model
 * (where it moved, else its model), in f32 without contraction - written by a pass of its own behind the primary rays, which runs only
 * while some mesh has such positions.  Several deformations between two frames leave "previous" at the earlier frame's state; a mesh
 * not deformed between two frames has no motion in the second; previous corners equal to the current ones bit for bit leave the pixel
 * as the primary rays wrote it; at enable time previous = current.  The planes are keyed by vertex id: hk_rebuild_mesh_tree may permute
 * triangles freely.  All deformation calls (single, batched, host and device sources) feed it; no deformation call gains a launch or a copy.
 * Stream-ordered like a deformation; enabling allocates (no wait), disabling frees the plane once the work enqueued has passed.
 * hk_upload_scene / hk_load_scene drop all motion state, hk_remove_meshes that of the removed meshes.
 * Refused with nothing written: an unknown mesh record (HK_E_INVALID), no scene (HK_E_NOT_READY). */
int hk_set_mesh_motion_vectors(hk_ctx* ctx, const HkMeshIndex* mesh, uint32_t enable);
/* hk_upload_scene for a FINISHED builder that may hold deferred meshes (hk_scene_builder_add_mesh_deferred): synchronous, like an upload.
 * Every pending tree - of a mesh no instance uses yet, too - is built on the device, straight into the mesh-level region in every
 * ordering the scene keeps, single-leaf navigators folded (the form hk_rebuild_mesh_tree writes); all pending meshes below 32 768
 * triangles are built TOGETHER, at a number of kernel launches that does not depend on how many there are, larger ones one by one on
 * the whole chip.  Meshes that were not pending go through the host layout untouched.
 *   HK_TREE_SAH   the mesh-level nodes equal, byte for byte in every ordering, those after hk_upload_scene of a twin builder that used
 *                 hk_scene_builder_add_mesh + hk_scene_builder_rebuild_mesh_tree on the same meshes.
 *   HK_TREE_LBVH  the Morton build: valid trees, not the host's.
 * The trees are written back into the builder in reference form (the mesh's nodes and its range of the concatenated array, in place:
 * the builder stays finished, the marks are cleared) and into the context's mirror, so the context is in the state hk_upload_scene
 * leaves: nothing is stale, hk_upload_materials / hk_upload_textures / hk_update_mesh_vertices work at once, the traversal mode is the
 * upload's.  A later load of the same builder builds only the trees of meshes deferred since.  A pending mesh of more than
 * HK_MESH_REBUILD_MAX_TRIANGLES triangles is completed by the host inside the call.
 * Argument errors (NULL, unknown mode: HK_E_INVALID; unfinished builder: HK_E_NOT_READY) write nothing; a failure after the upload has
 * begun leaves the context WITHOUT a scene (HK_E_NOT_READY at the next frame), never with stand-in trees. */
int hk_load_scene(hk_ctx* ctx, hk_scene_builder* b, uint32_t tree_mode);
/* Meshes added to the builder since the context last took its mesh level from it (hk_upload_scene, hk_load_scene, hk_add_meshes), appended
 * to the device scene without laying the scene out again.  The host adds them to the loaded builder (hk_scene_builder_add_mesh_deferred or
 * hk_scene_builder_add_mesh) and finishes it: the builder concatenates in id order, so every existing HkMeshIndex keeps its value and the
 * new ranges lie behind the old ones.  Instances of the new meshes - and materials appended on the builder - follow through
 * hk_update_scene_instances, which then lays out the instance level only.
 * A scene with two slots of the instance-level region (beyond the LDS copy) whose ordering count stays what it is: the mesh-level sub-arrays
 * (node planes per ordering, triangle and vertex planes, the wide records and ranks) keep capacities.  The new HkPrimitive / HkVertex
 * records go through the pinned staging pool of the deformations into the planes; deferred trees are built on the device as hk_load_scene
 * builds them (all below 32 768 triangles together, larger ones on the whole chip; above HK_MESH_REBUILD_MAX_TRIANGLES by the host inside
 * the call), trees the host built are threaded, boxed and folded for their ranges alone and sent through staging.  New ranges are in final
 * form whether an instance uses them yet or not.  When they do not fit, the scene moves ONCE to an allocation with every capacity at
 * least 1.5 times what is needed - both slots and every sub-array in one copy launch in stream order, existing wide records copied, not
 * derived again; the old allocation is freed once an event behind that copy has passed - polled only where a later call has waited for
 * the context's streams anyway (hipFree may wait for the device by itself), so until then it merely stays allocated.  No host wait for frames
 * in flight: the one wait is on the call's own build, whose ordering 0 is read back, unfolded into the builder (which stays finished,
 * marks cleared) and appended to the context's mirrors.  The cost follows the new meshes, plus one device-to-device move on growth.
 * Nothing of the existing meshes or of the instance level is read or rewritten: the call is accepted after hk_refit_scene_instances,
 * hk_rebuild_scene_trees, hk_update_materials, hk_update_mesh_vertices, hk_skin_mesh and hk_rebuild_mesh_tree; skins, deformed vertices,
 * rebuilt trees, wide records and the stale or fresh state of the mirrors stay as they were.  (hk_update_scene_instances is still refused
 * after a deformation: in that state the new meshes wait for their instances until the host's mirror is uploaded.)
 * A scene walked from the LDS copy (one slot), or an addition that changes the ordering count: the call does what hk_load_scene does for
 * the whole builder - small by definition; HK_E_NOT_READY when the mirrors are stale, as any re-layout.
 *   HK_TREE_SAH / HK_TREE_LBVH as in hk_load_scene: with HK_TREE_SAH the context holds, byte for byte, what hk_upload_scene of a twin
 *   builder that had every mesh from the start leaves.
 * With nothing new: HK_OK, nothing enqueued.  HK_E_INVALID with nothing written for NULL, an unknown mode, or a builder whose first meshes
 * are not the context's (counts of vertices, primitives and nodes, the HkMeshIndex records of the uploaded instances); HK_E_NOT_READY with
 * nothing written for no scene, an unfinished builder or one finished with stand-in instance trees.  A HIP failure before the scene
 * pointers are switched leaves the scene the context had; one after it leaves the context WITHOUT a scene, never with stand-in trees.
 * HkStats: scene_mesh_builds does not move, scene_device_tree_builds counts the meshes built. */
int hk_add_meshes(hk_ctx* ctx, hk_scene_builder* b, uint32_t tree_mode);
/* hk_add_meshes for meshes whose geometry lives in DEVICE memory (an iso-surface extracted on the GPU, a procedural terrain): the host
 * declares them by their counts (hk_scene_builder_declare_mesh), finishes the builder, and names their arrays here.  No array crosses to
 * the host on the caller's side and no HkPrimitive is assembled on a CPU thread; the builder GETS THE MESH BACK, as it gets the trees back.
 * After HK_OK the context, the builder and the mirrors are byte for byte what hk_add_meshes leaves for a twin builder that got the same
 * values through hk_scene_builder_add_mesh_deferred - every ordering's node plane, the triangle and vertex planes, wide records and
 * ranks where the scene has them, the builder's getters - so nothing is stale and every later call (deformations, rebuilds, instance
 * changes, removals, a second context or the bands taking the same builder through plain hk_add_meshes) works unchanged.  Meshes added to
 * the builder the ordinary way since the last add travel in the same call; n == 0 with no unresolved mesh IS hk_add_meshes.  Accepted in
 * every state hk_add_meshes is accepted in.
 *   sources[i]: mesh_id - a declared, still unresolved mesh of the builder; every unresolved mesh must be named by exactly one source.
 *   positions / normals (required) / uvs (or NULL = (0, 0)): device memory, 3 / 3 / 2 floats per vertex at pointer + v * stride; a
 *   stride of 0 means packed (12 / 12 / 8), otherwise it is at least that and a multiple of 4 - a column slice of a wider row costs no
 *   copy.  indices: n_indices x uint32, contiguous; NULL iff the mesh was declared with n_indices == 0.  flags and _pad must be 0.
 * Phase 0, on the host, checks the whole batch before anything is enqueued (the failing source's index is in hk_last_error()): every
 * check of hk_add_meshes; the mesh ids; pointers 4-byte aligned, memory of the context's device or mapped host memory, the whole extent
 * - (n_vertices - 1) * stride + 12 (or + 8), n_indices * 4 - inside its allocation; strides; flags.  HK_E_INVALID, nothing written.
 * Phase 1, on the device, is ONE launch however many sources there are: the context's stream waits for an event recorded on
 * producer_stream (NULL: the caller has ordered itself, the rule of hk_deform_meshes_device), k_assemble_meshes writes the HkVertex and
 * HkPrimitive records of all sources into a device block of the context's and a status word, and an event behind it goes back to the
 * producer stream, which may then write the sources again.  Values move as bits.  An index >= n_vertices is never followed (vertex 0 is
 * read instead) and flags its source.  The host waits for the stream - hk_add_meshes goes behind every enqueued frame and waits for its
 * own build anyway - and reads status and block back in one copy: a flagged source returns HK_E_INVALID naming the lowest one, with the
 * scene, the mirrors and the builder unchanged and the meshes still unresolved.
 * Phase 2: the builder takes the records (the mesh box from the read-back positions with add_mesh's arithmetic); unresolved is cleared,
 * pending stays.  Phase 3 is the body of hk_add_meshes itself: where it appends on the device, the ranges of these meshes are fed from the
 * device block and only the records of meshes the host added go through pinned staging; where it lays the scene out again (the LDS copy,
 * a changed ordering count) the builder is complete and nothing is special.  Trees, write-back, relocation and the host's completion of
 * meshes above HK_MESH_REBUILD_MAX_TRIANGLES are hk_add_meshes'.
 * There is no hk_multi_ form: a device pointer lives on one device.  A second context, or the other bands, take the completed builder
 * through hk_add_meshes / hk_multi_add_meshes. */
typedef struct HkMeshSource {
  uint32_t mesh_id;
  uint32_t flags;               /* must be 0 */
  const void* positions;        /* DEVICE memory */
  const void* normals;
  const void* uvs;              /* or NULL */
  const void* indices;          /* or NULL */
  uint32_t positions_stride, normals_stride, uvs_stride;   /* bytes; 0 = packed */
  uint32_t _pad;
} HkMeshSource;                 /* 56 bytes */
int hk_add_meshes_device(hk_ctx* ctx, hk_scene_builder* b, const HkMeshSource* sources, uint32_t n, uint32_t tree_mode, void* producer_stream);
/* Meshes removed from the loaded scene: the mesh-level region compacted on the device (scene_remove.hip; DESIGN 3 "Meshes that leave").
 * removed[0..n) are the extents hk_scene_builder_remove_mesh returned since the builder's last finish - all in the context's CURRENT
 * layout, so one call per builder finish, in order; entries with node_count 0 are skipped, and with nothing left to do the call returns
 * HK_OK with nothing enqueued.  The host removes the instances of those meshes first (hk_update_scene_instances).  Calls after the
 * removal name the survivors by their new records (hk_scene_builder_mesh_index after the finish, or hk_rebase_mesh_index).
 * A scene with two slots of the instance-level region whose ordering count stays what it is: the scene moves, behind every stream and
 * without a host wait, to a NEW allocation whose capacities follow the survivors (1.5 times what is needed) - ONE compaction launch
 * however many meshes go moves the surviving runs of every node plane, the triangle and vertex planes and the wide records and ranks,
 * a small launch beside it copies the instance-level slot and rebases the three mesh offsets of every instance record, and one in front
 * of both copies the plan (planes and run lists) from pinned to device memory.  Frames in
 * flight go on reading the old allocation, which is freed behind an event; skins, morph sets, deformed vertices, rebuilt trees and wide
 * records of the survivors stay as they are, those of the removed meshes are freed behind the same event.  Accepted in every state
 * hk_add_meshes is accepted in (mirrors stale or fresh); a pending propagate of deformed boxes goes first.
 * A scene walked from the LDS copy (one slot), or a removal that changes the ordering count: the mirrors are compacted and the scene is
 * laid out again on the host; HK_E_NOT_READY with NOTHING changed when the mirrors are stale or a mesh was deformed, as any re-layout.
 * Afterwards the context holds, byte for byte, what hk_upload_scene of a twin builder that never had the meshes leaves (given the same
 * device-side edits).  Everything is validated before anything is written or enqueued; the failing entry's index is in hk_last_error().
 * HK_E_INVALID: NULL with n > 0; an extent beyond the mirrors; n_primitives 0 or node_count != 3 n_primitives - 2; two extents that
 * overlap in a range or are ordered differently in the three ranges; an uploaded instance whose mesh lies inside an extent; an extent
 * that cuts a mesh the context knows (an instance's record, a deformable mesh, a mesh with wide records) partly; extents that would leave
 * the scene without a mesh (a scene holds at least one: load another scene instead).  HK_E_NOT_READY: no
 * scene.  A HIP failure before the scene pointers are switched leaves the scene intact, one after it leaves the context WITHOUT a scene.
 * HkStats: scene_mesh_builds does not move on the device path. */
int hk_remove_meshes(hk_ctx* ctx, const HkMeshExtent* removed, uint32_t n);
int hk_upload_textures(hk_ctx* ctx, const HkImageDesc* images, uint32_t n_images);
/* New texels and sampler fields for ONE uploaded texture of the same width and height (an animated texture; hk_upload_textures replaces
 * the whole array behind a host wait).  The texels go through the pinned staging pool of the deformations and land in place in the
 * texel buffer, behind every enqueued kernel that can read texels on whichever stream (the context's events: no host wait); the 16-B
 * descriptor (sRGB flag, address modes, filter) is rewritten in the slot in use - in both slots of a two-slot scene.  Works whatever
 * was changed on the device before (refits, tree rebuilds, deformations).  HK_E_INVALID with nothing written for NULL, index >= the
 * uploaded count, a size that differs or an address mode out of range; HK_E_NOT_READY when no textures have been uploaded. */
int hk_update_texture(hk_ctx* ctx, uint32_t index, const HkImageDesc* image);
/* Texture edits whose SOURCES LIE IN DEVICE MEMORY (a video frame decoded on the GPU, a procedural or learned texture in a tensor, a
 * lightmap a kernel wrote), MANY per call: whole textures or sub-rectangles, 8-bit or floating point, strided.  After the call the
 * texel buffer and the texture descriptors - in both slots of a two-slot scene - hold, byte for byte, what hk_update_texture would have
 * left, given per texture the current texels with the rectangles replaced by hk_encode_texels of the same values.  One kernel launch
 * whatever n is; only the item table travels through the pinned staging pool, the sources are read where they lie.
 *   Sources.  Element (x, y, ch) of an item lies at data + y * stride_y + x * stride_x + ch * stride_c (bytes; multiples of the element
 * size; 0 = a broadcast): a torch tensor in HWC or CHW order, a slice of one or an expanded one, without a copy.  channels 1 = grey
 * (rgb take the value, alpha 255), 3 = rgb (alpha 255), 4 = rgba.  Row 0 is v = 0, as in HkImageDesc.
 *   Conversion, per element, in f32, without contraction.
 *     HK_TEXELS_U8   the byte is taken as it is (it is already in the texture's encoding).
 *     HK_TEXELS_F16  the half is widened exactly to f32, then as F32.
 *     HK_TEXELS_F32  without HK_TEXTURE_LINEAR_SOURCE the float IS the encoded value: NaN -> 0, v = min(max(x, 0), 1),
 *                    byte = (uint32_t)(v * 255.0f + 0.5f), the product and the sum two separately rounded f32 operations.
 *     HK_TEXTURE_LINEAR_SOURCE (float sources only; on a U8 item HK_E_INVALID): the rgb channels of a texture whose sRGB bit is set
 *                    after this call are LINEAR light and are encoded: v clamped as above, byte = the number of k in 1 .. 255 with
 *                    v > mid[k], mid[k] = (float)(((double)lut[k - 1] + (double)lut[k]) / 2), lut the 256-entry sRGB decode table the
 *                    samplers read (the sRGB EOTF in double, rounded once).  Comparisons only: encode(lut[b]) == b for every b.  Alpha,
 *                    and every channel of a texture that is not sRGB, take the plain rule.
 *   Sampler.  With HK_TEXTURE_SET_SAMPLER the item's is_srgb / address_u / address_v / filter_linear replace the texture's; otherwise the
 * descriptor stays as it is and those fields are not read.
 *   Ordering.  The rule of hk_update_texture and hk_deform_meshes_device: the texel buffer has one copy, so the write goes behind every
 * frame enqueued on every stream that reads texels - no host wait.  With producer_stream (a hipStream_t) != NULL the context's stream
 * first waits for an event recorded there at the call, and the producer then waits for an event recorded behind the kernel that reads
 * the sources: the caller may overwrite them in stream order right after the call.  NULL: the caller has ordered itself.  If an
 * hk_upload_textures is still pending, the call lays the scene out first, as the next frame would (HK_E_NOT_READY without a complete
 * scene).
 *   Validation.  The whole batch before anything is enqueued; a refused call writes nothing.  HK_E_INVALID for: NULL ctx, or NULL items
 * with n > 0; an index >= the uploaded count; an unknown format, flag bit or channel count; a rectangle that is empty or leaves the
 * texture; a stride that is no multiple of the element size; an address mode out of range under HK_TEXTURE_SET_SAMPLER; two items of one
 * call whose rectangles in the same texture overlap (one launch cannot order them); a source that is misaligned for its element size,
 * neither memory of the context's device nor host memory mapped for it (pageable memory is refused: a mistaken pointer cannot fault the
 * device), or whose extent - computed from the strides - leaves its allocation.  HK_E_NOT_READY when no textures have been uploaded.
 * n == 0: HK_OK, nothing enqueued.
 *   State.  Afterwards the context's host copy of the touched textures is stale (a mark per texture).  Nothing reads that copy until
 * hk_upload_textures replaces all of it, and an hk_update_texture of a texture refreshes its copy: NO CALL IS NEWLY REFUSED after this one.
 * There is no hk_multi_ form, as hk_deform_meshes_device and hk_set_instance_transforms_device have none: a device pointer lives on one device. */
#define HK_TEXELS_U8  0u   /* unsigned bytes, already in the texture's encoding */
#define HK_TEXELS_F16 1u   /* IEEE half, widened exactly to f32, then as F32 */
#define HK_TEXELS_F32 2u
#define HK_TEXTURE_SET_SAMPLER   1u  /* take is_srgb / address_u / address_v / filter_linear from the item; otherwise the descriptor stays */
#define HK_TEXTURE_LINEAR_SOURCE 2u  /* float sources only: rgb of an sRGB texture is LINEAR light and is encoded (rule above) */
typedef struct HkTextureSource {
  uint32_t    index;           /* an uploaded texture */
  uint32_t    format;          /* HK_TEXELS_* */
  const void* data;            /* DEVICE memory (or host memory mapped for the device); hk_encode_texels: HOST memory */
  uint64_t    stride_x, stride_y, stride_c;  /* bytes; multiples of the element size; 0 allowed (a broadcast) */
  uint32_t    channels;        /* 1 (grey -> rgb, alpha 255), 3 (alpha 255) or 4 */
  uint32_t    x0, y0, width, height;  /* the rectangle of the texture that is written; inside the texture, width, height >= 1 */
  uint32_t    flags;           /* HK_TEXTURE_SET_SAMPLER | HK_TEXTURE_LINEAR_SOURCE */
  uint32_t    is_srgb, address_u, address_v, filter_linear;  /* read with HK_TEXTURE_SET_SAMPLER */
} HkTextureSource;             /* 80 bytes, no implicit padding: 8-byte members at 8, 16, 24, 32, then ten 4-byte members */
int hk_update_textures_device(hk_ctx* ctx, const HkTextureSource* items, uint32_t n, void* producer_stream);
/* ... and the way back: waits for the context's streams, then copies the texels the device holds of texture `index` to `rgba8` (bytes
 * must be width * height * 4, else HK_E_INVALID; HK_E_NOT_READY when no textures have been uploaded).  Refreshes the context's host copy
 * of the texture and clears its mark. */
int hk_read_texture(hk_ctx* ctx, uint32_t index, uint8_t* rgba8, size_t bytes);
/* The host twin of the kernel's conversion, no GPU needed: one item's rectangle, read from HOST memory laid out the same way, to
 * width * height * 4 bytes (row-major, rgba).  texture_is_srgb: the texture's sRGB bit AFTER the call the item would be part of.  index,
 * x0, y0 and the sampler fields are not read.  HK_E_INVALID for NULL, an unknown format, flag bit or channel count, an empty
 * rectangle, a stride that is no multiple of the element size, a misaligned pointer, HK_TEXTURE_LINEAR_SOURCE on a U8 item. */
int hk_encode_texels(const HkTextureSource* item, uint32_t texture_is_srgb, uint8_t* rgba8_out);
/* InstanceRenderAssets::set + write_buffer, instance.rs:82-108 */
int hk_upload_instances(hk_ctx* ctx, const HkInstance* instances, uint32_t n_instances, const HkNode* instance_nodes,
                        uint32_t n_instance_nodes, const HkEmissive* emissives, uint32_t n_emissives,
                        const HkNode* emissive_nodes, uint32_t n_emissive_nodes, const HkAliasEntry* alias_table,
                        uint32_t n_alias);
/* PreviousMeshUniform::transform per instance (instance.rs:111-128; prepass.wgsl:50,96):
 * n_instances x 16 floats, column-major, the model matrices of the PREVIOUS frame.  Optional: without
 * it every instance is static (previous = current).  Applies to the instances of the last
 * hk_upload_instances call and is dropped by the next one, so a host with moving objects uploads both
 * every frame, as the reference extracts both every frame. */
int hk_upload_previous_transforms(hk_ctx* ctx, const float* models, uint32_t n_instances);
/* convenience: the three uploads above from a finished builder */
int hk_upload_scene(hk_ctx* ctx, const hk_scene_builder* b);
/* convenience: hk_upload_instances + hk_upload_previous_transforms from a re-finished builder whose
 * meshes and materials are unchanged.  Only the instance-level device arrays are rewritten. */
int hk_upload_scene_instances(hk_ctx* ctx, const hk_scene_builder* b);
/* NoiseTextures, lib.rs:189-219,515-598: 16 tiles of 64x64 RGBA8, tile-major */
int hk_upload_noise(hk_ctx* ctx, const uint8_t* rgba, size_t bytes);
/* prepare_light_textures / prepare_prepass_textures / post-process textures: (re)allocate all
 * screen-space resources and ZERO the 10 reservoir buffers (light.rs:307-383). */
int hk_resize(hk_ctx* ctx, uint32_t width, uint32_t height, float upscale_ratio);

/* ------------------------------------------------------------------ per-frame */
/* the four dynamic uniforms of bind group 0 (prepass.rs:546-553) */
/* TAA / upscale variant that selects the prepass sub-pixel jitter (prepass.rs:489-490,
 * prepass.wgsl:30-38), and Upscale::sharpness() (lib.rs:489-496) that HK_PASS_FSR_RCAS reads;
 * hk_frame_stage sets all three from HkSettings, hk_pass_run uses the last values. */
int hk_set_view_options(hk_ctx* ctx, uint32_t taa, uint32_t upscale_kind, float upscale_sharpness);
int hk_frame_begin(hk_ctx* ctx, const HkFrame* frame, const HkView* view, const HkPreviousView* previous_view,
                   const HkLights* lights);
/* One dispatch over rows [row_begin,row_end) of its grid (row_end = 0 means "all rows").  The
 * reservoir ping-pong (light.rs:376,480-481,518-546) follows frame.number of hk_frame_begin. */
int hk_pass_run(hk_ctx* ctx, uint32_t pass, uint32_t arg, uint32_t row_begin, uint32_t row_end);
/* The node order of the reference for the band of this context (whole image by default):
 *   TEMPORAL     = PrepassNode::run + LightNode::run up to and including the temporal dispatches
 *   SPATIAL      = the spatial_reuse dispatches of LightNode::run (light.rs:689-697)
 *   POST_PROCESS = PostProcessNode::run denoise loop + tone mapping (post_process.rs:1190-1234)
 * flags bit0: the G-buffer was supplied by the host (hk_write_buffer), skip the primary-ray prepass. */
#define HK_FRAME_EXTERNAL_GBUFFER 1u
/* flags bit1 (hk_frame_render): also run HK_STAGE_ANTIALIAS */
#define HK_FRAME_ANTIALIAS 2u
/* flags bit2 (hk_frame_render, hk_multi_frame_render): hk_balance_bands right after hk_frame_begin - split THIS frame's rows by
 * cost and keep the split from here on.  Rows that change owner find the new owner's (stale) reservoirs as history: use it on
 * the first frame, after a cut, or accept a few frames of re-convergence in the moved rows. */
#define HK_FRAME_BALANCE_BANDS 4u
/* flags bit3 (hk_frame_render with a communicator, hk_multi_frame_render): after the last stage, band 0 collects the other bands' rows of
 * the frame's final image (hk_final_buffer) - SURVEY 8e step 7, hk_comm_gather / hk_multi_gather.  With a communicator and without
 * HK_FRAME_ANTIALIAS the rows travel WHILE the next frame renders (ABI 7: every RCCL call runs on a stream of the communicator's own,
 * ordered against the context's stream by events; the tone-mapped image is double-buffered by frame parity): the image on band 0 is
 * complete once hk_frame_wait, any buffer access, or the hk_frame_begin of the frame after next has been passed. */
#define HK_FRAME_GATHER 8u
/* flags bit4 (hk_frame_render; round 6): take THIS frame's band time - HIP events on the context's stream around stage TEMPORAL and
 * around stage SPATIAL, i.e. the band's own work on the critical cycle of a sharded frame WITHOUT the waits for its neighbours' halos
 * in between (with a communicator every band's wall clock shows the slowest band's time; this does not) - for hk_band_time_ms. */
#define HK_FRAME_TIME_BAND 16u
int hk_frame_stage(hk_ctx* ctx, uint32_t stage, const HkSettings* settings, uint32_t flags);
/* hk_frame_begin + TEMPORAL, SPATIAL, POST_PROCESS (+ ANTIALIAS with HK_FRAME_ANTIALIAS): single GPU, no halo exchange */
int hk_frame_render(hk_ctx* ctx, const HkFrame* frame, const HkView* view, const HkPreviousView* previous_view,
                    const HkLights* lights, const HkSettings* settings, uint32_t flags);
int hk_frame_wait(hk_ctx* ctx);

/* ------------------------------------------------------------------ present (the reference's OverlayNode, overlay.rs:311-395) */
/* The one step between the internal rgba16f image and what the camera's view target receives (overlay.wgsl:28-48).  Per target
 * pixel, in f32 under the numeric contract:
 *   c   = the final image (hk_final_buffer(settings, frame_flags)) at the pixel: the texel itself when the plane has the target's
 *         size, otherwise the bilinear clamp-to-edge sample at uv = ((x + 0.5) / width, (y + 0.5) / height)
 *   c   = the albedo of the frame last rendered, sampled the same way, where any of c's four components is NaN
 *   HK_PRESENT_HDR: l = dot(c.rgb, (0.2126, 0.7152, 0.0722)); l' = clamp(l, 0.0005, 0.995); c.rgb *= (l' / (1 - l')) / l
 *         (inverse_reintard_luminance; a black texel gives 0 * inf = NaN, as in the reference)
 *   d   = clear (HK_PRESENT_CLEAR) or the target's current content decoded to linear (overlay.rs:365-370)
 *   out = (c.rgb * c.a + d.rgb * (1 - c.a), c.a + d.a * (1 - c.a))          BlendState::ALPHA_BLENDING, overlay.rs:133
 * encoded to the target's format.  The 8-bit formats encode colour with the sRGB curve and every channel as
 * floor(0.5 + 255 * clamp(v, 0, 1)) (a NaN becomes code 0) and decode colour with the material textures' sRGB table. */
#define HK_FORMAT_RGBA16F 0u
#define HK_FORMAT_RGBA32F 1u
#define HK_FORMAT_RGBA8_UNORM_SRGB 2u
#define HK_FORMAT_BGRA8_UNORM_SRGB 3u /* bevy's TextureFormat::bevy_default() */
#define HK_PRESENT_HDR 1u   /* the view target is HDR: undo the Reinhard-luminance tone map */
#define HK_PRESENT_CLEAR 2u /* blend over `clear` instead of the target's content */
typedef struct HkPresentTarget {
  void* ptr;            /* device memory the host owns (a torch tensor, an imported swapchain image), aligned to the pixel size */
  uint32_t width, height;
  uint32_t pitch_bytes; /* >= width * bytes per pixel, a multiple of the pixel size */
  uint32_t format;      /* HK_FORMAT_* */
  uint32_t flags;       /* HK_PRESENT_HDR | HK_PRESENT_CLEAR */
  float clear[4];       /* linear rgba, read under HK_PRESENT_CLEAR */
} HkPresentTarget;
/* Rows [row_begin, row_end) of the target, asynchronously like hk_frame_render: the kernel runs behind everything that writes the
 * final image and the albedo of the frame last begun (the post stream and a pending gather included), and the kernels of the frames
 * that follow wait for it before they write a plane it reads - through the context's events, never through a host wait.
 * hk_frame_wait returns once the target is written.  Refused with nothing written: a NULL or misaligned target or pitch, an unknown
 * format or flag, row_begin > row_end or row_end > height (HK_E_INVALID); no hk_frame_begin yet (HK_E_NOT_READY); a context that is
 * one band of several (HK_E_UNSUPPORTED: a band holds its own rows of the albedo only).
 * The target must not overlap any of the context's own planes (hk_device_ptr): the kernel reads the final image and the albedo as
 * memory nothing else writes while it runs. */
int hk_present(hk_ctx* ctx, const HkSettings* settings, uint32_t frame_flags, const HkPresentTarget* target, uint32_t row_begin,
               uint32_t row_end);

/* ------------------------------------------------------------------ ray queries (picking, line of sight, probe rays) */
/* Rays of the host's own against the scene the context holds: what is under a cursor ray, is B visible from A, where does a probe
 * land.  One record in, one record out, in the order given; no hk_resize, no frame and no band is involved, and a context that is one
 * band of several answers like a single context (it holds the whole scene).
 *   direction      used as given, NOT normalised; `distance` is in units of it (position = origin + distance * direction), as in the
 *                  reference's traverse_top (light.wgsl:442-486).  There is no t_min: offset the origin.
 *   max_distance   hits at or beyond it are not reported (+inf and 3.4e38 mean "any")
 *   exclude_instance  an instance the ray passes through; 0xFFFFFFFF excludes nothing
 * A miss has distance = max_distance, instance = primitive = 0xFFFFFFFF and status HK_RAY_MISS - what the reference's Hit holds.
 * A ray is HK_RAY_INVALID, and is not walked, when a component of origin or direction is not finite, when direction is all zero, or
 * when max_distance is NaN or negative: it is written as a miss with that status, decided per ray before any walk, and the rays
 * around it are answered as usual.
 * flags:
 *   HK_RAYS_CLOSEST     the closest hit: the reference's traverse_top with early_distance = 0.  A context created with
 *                       HK_CTX_EXACT_TRAVERSAL walks the reference's order and reports the reference's hit bit for bit; otherwise the
 *                       walk is the one the frame's own closest-hit rays take on this scene (hk_traversal_mode), and the hit is the
 *                       reference's except where two candidates tie or a box is grazed within rounding.
 *   HK_RAYS_ANY         occlusion only: the walk stops at the first hit it meets (early_distance = +inf).  status says hit or miss;
 *                       WHICH hit the record names, and its distance, are not promised.  Never the wide walk.
 *   HK_RAYS_ATTRIBUTES  closest hits only: material, uv and normal are filled as the light passes see the hit (hit_info,
 *                       light.wgsl:496-523: interpolated uv, interpolated normal through the inverse-transpose model, normalised; a miss
 *                       has material 0xFFFFFFFF and zeros).  Without the flag the three fields are zero.
 *   HK_RAYS_STACKLESS   never take the wide walk: scenes beyond the LDS copy are walked by skip links in the ray's ordering even where
 *                       hk_traversal_mode reports HK_TRAVERSAL_WIDE.  (A pending subtree the wide walk has to drop is counted in
 *                       HkStats.wide_stack_lost, as in frames.) */
typedef struct HkRay {
  float origin[3];
  float max_distance;
  float direction[3];
  uint32_t exclude_instance;
} HkRay; /* 32 bytes */
typedef struct HkRayHit {
  float distance;
  uint32_t instance, primitive, material;
  float barycentric[2]; /* of the hit inside its triangle: position = v0 + b[0] * (v1 - v0) + b[1] * (v2 - v0) */
  float uv[2];
  float normal[3];
  uint32_t status; /* HK_RAY_* */
} HkRayHit; /* 48 bytes */
#define HK_RAYS_CLOSEST 0u
#define HK_RAYS_ANY 1u
#define HK_RAYS_ATTRIBUTES 2u
#define HK_RAYS_STACKLESS 4u
#define HK_RAY_MISS 0u
#define HK_RAY_HIT 1u
#define HK_RAY_INVALID 2u
/* `rays` and `hits` in host memory: the same launch between two copies through pinned staging; returns when `hits` is written.
 * n = 0 is HK_OK and launches nothing.  HK_E_INVALID (nothing written): a NULL context, a NULL pointer with n > 0, an unknown flag bit,
 * HK_RAYS_ATTRIBUTES together with HK_RAYS_ANY.  HK_E_NOT_READY: no scene uploaded. */
int hk_cast_rays(hk_ctx* ctx, const HkRay* rays, uint32_t n, uint32_t flags, HkRayHit* hits);
/* `d_rays` (n x 32 bytes) and `d_hits` (n x 48 bytes) in device memory, both aligned to 16 bytes: enqueued on the context's main
 * stream (hk_stream) with no wait - behind every scene upload, refit, rebuild, deformation and frame enqueued before it, reading the
 * instance-level slot the next frame would read.  The caller orders its own stream against hk_stream (or calls hk_frame_wait). */
int hk_cast_rays_device(hk_ctx* ctx, const void* d_rays, uint32_t n, uint32_t flags, void* d_hits);

/* ------------------------------------------------------------------ band sharding (multi-GPU) */
/* Restrict this context to band `band_index` of `band_count` horizontal bands of the render image
 * (bands are contiguous row ranges, remainder rows spread over the first bands). */
int hk_set_band(hk_ctx* ctx, uint32_t band_index, uint32_t band_count);
int hk_band_rows(uint32_t height, uint32_t band_index, uint32_t band_count, uint32_t* row_begin, uint32_t* row_end);
/* Bands of unequal height (round 3).  Equal row counts are equal WORK only when the rows are alike: a sky band of the city-class
 * 4K frame takes 0.3 ms, a band full of buildings 6.3 ms.  bounds[0] = 0 < bounds[1] < ... < bounds[band_count] = the scaled render
 * height: band i renders rows [bounds[i], bounds[i + 1]).  Every rank of a sharded frame must set the SAME boundaries (the halo
 * schedules are derived from them on each rank); NULL / 0 returns to the equal split; hk_set_band with another band count and
 * hk_resize drop them.
 *   hk_row_costs           geometry pixels (depth >= epsilon) per full-size row of the frame most recently begun.  A rank that
 *                          ray-casts the WHOLE frame's primary rays once (hk_frame_begin + hk_pass_run(HK_PASS_PREPASS, 0, 0, 0))
 *                          holds what every other rank holds, bit for bit, so all ranks derive the same split without talking.
 *   hk_balanced_band_bounds  pure host logic: boundaries that give every band about the same cost, cost(row) = its geometry
 *                          pixels + width x background_cost, at least min_rows rows per band; row_cost has cost_rows entries
 *                          (hk_row_costs: the full-size height).  hk_balance_bands uses 1/4 for scenes walked from LDS (cheap
 *                          geometry pixels: the Cornell box) and 1/16 beyond (profiles/r03_band_balance_probe.json).
 *   hk_balance_bands       the three steps in one call, after hk_frame_begin: full-frame primary rays, count, split, set on this
 *                          context (min_rows 0 = 8, never more than rows / bands); bounds_out (optional) receives the split.  Deterministic across ranks. */
int hk_set_band_bounds(hk_ctx* ctx, const uint32_t* bounds, uint32_t n_bounds /* band_count + 1 */);
int hk_get_band(hk_ctx* ctx, uint32_t* band_index, uint32_t* band_count); /* what hk_set_band set (either pointer may be NULL) */
int hk_get_band_bounds(hk_ctx* ctx, uint32_t* bounds, uint32_t n_bounds /* band_count + 1 */); /* the split in force (explicit or equal) */
int hk_balance_bands(hk_ctx* ctx, uint32_t min_rows, uint32_t* bounds_out, uint32_t n_bounds /* band_count + 1, or 0 with NULL */);
int hk_row_costs(hk_ctx* ctx, uint32_t* geometry_pixels_per_row, uint32_t n_rows /* = the full-size height */);
int hk_balanced_band_bounds(const uint32_t* row_cost, uint32_t cost_rows, uint32_t width, uint32_t render_rows, uint32_t band_count,
                            uint32_t min_rows, float background_cost /* of a background pixel, geometry pixel = 1; <= 0: 1/16 */, uint32_t* bounds);
/* Bands of equal MEASURED time (round 6).  The split by geometry pixels prices every geometry pixel alike; the rows of a city-class
 * frame differ three times in walk length, and part of a band's time is fixed cost.  So: every M frames each rank takes its band's
 * GPU time (hk_frame_render(.., HK_FRAME_TIME_BAND), hk_band_time_ms), the ranks all-gather these N floats over the host's channel,
 * and every rank evaluates the same pure function on them:
 *   hk_rebalanced_band_bounds  bounds[band_count + 1] in force + band_ms[band_count] -> out[band_count + 1]: the boundaries moved
 *                          `damping` (0..1] of the way towards equal times (a band's time spread over its rows evenly, or by the
 *                          optional prior row_weight[render_rows], e.g. geometry pixels per row), at most max_shift rows per call
 *                          (0: no limit), at least min_rows per band.  A band without a usable time keeps the split as it is.
 *   hk_band_migration_plan / _schedule  what must travel when the split changes between two frames: the rows of the history
 *                          reservoirs (the three temporal outputs + the spatial outputs whose pass is on: what frame
 *                          `next_frame_number` reads as history) that change owner, from the band that owned them under old_bounds to
 *                          the band that owns them under new_bounds (NULL = the equal split) - the same row plan / one global order
 *                          of sends and receives as hk_band_plan / hk_band_schedule.  After it every band holds, for the rows it now
 *                          owns, exactly what their previous owner held: the sharded frames that follow equal the single context bit
 *                          for bit as before.  (The anti-aliasing tail keeps more per-pixel state - previous tone-mapped / TAA /
 *                          G-buffer planes: with it keep the split, or treat a re-split as a cut.)
 *   hk_migrate_bands       with a communicator: the migration as one RCCL exchange on the communicator's stream, ordered behind
 *                          everything the context has enqueued, then hk_set_band_bounds(new_bounds).  Every rank calls it with
 *                          the same arguments, between two frames.  (A host with its own transport moves hk_band_migration_schedule's
 *                          rows and calls hk_set_band_bounds itself; hk_multi_migrate_bands is the one-process form.) */
int hk_rebalanced_band_bounds(const uint32_t* bounds, const float* band_ms, uint32_t band_count, uint32_t render_rows, const float* row_weight /* or NULL */,
                              uint32_t min_rows, uint32_t max_shift, float damping, uint32_t* out);
int hk_band_migration_plan(uint32_t width, uint32_t height, float upscale_ratio, const uint32_t* old_bounds, const uint32_t* new_bounds, uint32_t band_index,
                           uint32_t band_count, uint32_t next_frame_number, const HkSettings* settings, HkHaloOp* ops, uint32_t* n_ops);
int hk_migrate_bands(hk_ctx* ctx, const uint32_t* new_bounds, uint32_t n_bounds /* band_count + 1 */, uint32_t next_frame_number, const HkSettings* settings);
/* the band time of the last frame rendered with HK_FRAME_TIME_BAND, in ms (waits for that frame's spatial stage; HK_E_NOT_READY if none) */
int hk_band_time_ms(hk_ctx* ctx, float* ms);
/* Halo transfers that must complete before `stage` runs on this context.  Pure host logic.
 * ops may be NULL to query the count.
 * Moving cameras / objects: the temporal and spatial dispatches read LAST frame's reservoirs at reprojected
 * positions (light.wgsl:1091,1144,1404,1525), which can lie up to |velocity| rows inside a neighbouring band.
 * Passing HK_STAGE_TEMPORAL_WITH_HISTORY(rows) as the stage returns "exchange C": `rows` rows of the
 * reservoir buffers frame n reads as history (the temporal outputs of all three channels and the spatial
 * outputs that are enabled), to be received before stage TEMPORAL of frame n.  A reprojection that lands
 * beyond the halo reads the local, stale rows - the documented deviation; rows = 0 (static camera) is
 * plain HK_STAGE_TEMPORAL and has no transfers. */
#define HK_STAGE_TEMPORAL_WITH_HISTORY(rows) ((uint32_t)HK_STAGE_TEMPORAL | ((uint32_t)(rows) << 8))
/* ... and the scatter stores of frame n's temporal dispatches that cross a band border (ABI 7).  A pixel of
 * band B whose history reservoir was rejected stores it at the reprojected slot of previous_spatial, up to `rows` rows away - in
 * the rows of a neighbour, whose spatial pass reads that slot - and B's own spatial pass reads slots up to `rows` rows outside B
 * that pixels of OTHER bands store to.  With a history halo the temporal dispatches of a band therefore PARK their stores
 * (HK_BUF_PARKED_TO0 / _RECORD0 + channel) and HK_STAGE_SPATIAL_WITH_HISTORY(rows) adds to exchange A, for every channel whose
 * spatial pass is enabled (sun and emissive share their spatial buffers: both, in dispatch order), 2 x rows rows of the parked
 * planes per side: every store that can reach a slot the band reads comes from a pixel at most 2 x rows rows outside it.  Stage
 * SPATIAL then resolves them - the highest storing pixel index wins, the rule HK_CTX_DETERMINISTIC_SCATTER and the oracle apply
 * to the reference's write-write race - before spatial_reuse runs: the union of the bands equals the single context bit for bit
 * under camera and object motion. */
#define HK_STAGE_SPATIAL_WITH_HISTORY(rows) ((uint32_t)HK_STAGE_SPATIAL | ((uint32_t)(rows) << 8))
/* How many history rows does this frame need?  Pure host logic, the same number on every rank (all of them hold the same
 * uniforms and the same scene).  Returns in *rows an upper bound of |row of the reprojected pixel - row of the pixel| over every
 * surface point the frame can show: the reprojection is previous_uv = uv - velocity with velocity = clip_to_uv(view_proj x p) -
 * clip_to_uv(previous_view_proj x p_previous) (prepass.wgsl:94-95), i.e. in NDC a projective map M = previous_view_proj x T x
 * inverse_view_proj of the pixel's own (x, y, depth), T = identity for static geometry and previous_model x model^-1 for an
 * instance that moved.  The bound is taken over the NDC box of the scene's world bounds (static part) and of every moved box with
 * interval arithmetic on y x (M v).w - (M v).y in centred form over a grid of cells, divided by the smallest (M v).w of the cell;
 * cells whose reprojection is certainly off screen do not count (the temporal kernels neither load nor store there).  + 2 rows
 * for the sub-pixel jitter of the deferred texel and the truncation to a row index, rounded up to a multiple of 4 (schedules are
 * cached per row count).  0 when the view did not change and nothing moved.  A reprojection that cannot be bounded (the previous
 * camera's plane cuts through the visible volume) gives render_rows: every band then needs all of last frame's rows. */
typedef struct HkMovedBox {
  float min[3];
  float _pad0;
  float max[3];
  float _pad1;
  float previous_from_current[16]; /* previous_model x model^-1, column-major: where a point of the box was last frame */
} HkMovedBox;
int hk_history_rows_bound(const HkView* view, const HkPreviousView* previous_view, uint32_t render_rows, const float scene_min[3],
                          const float scene_max[3], const HkMovedBox* moved, uint32_t n_moved, uint32_t* rows);
int hk_band_plan(hk_ctx* ctx, uint32_t stage, const HkSettings* settings, HkHaloOp* ops, uint32_t* n_ops);
/* Same plan without a context (used by hosts that only schedule): */
int hk_band_plan_for(uint32_t width, uint32_t height, float upscale_ratio, uint32_t band_index, uint32_t band_count,
                     uint32_t stage, uint32_t frame_number, const HkSettings* settings, HkHaloOp* ops, uint32_t* n_ops);
/* ... with an explicit split (bounds: band_count + 1 scaled render rows, see hk_set_band_bounds; NULL = hk_band_plan_for) */
int hk_band_plan_bounds(uint32_t width, uint32_t height, float upscale_ratio, const uint32_t* bounds, uint32_t band_index,
                        uint32_t band_count, uint32_t stage, uint32_t frame_number, const HkSettings* settings, HkHaloOp* ops,
                        uint32_t* n_ops);

/* One side of a halo transfer, as the executor needs it: a byte range of a buffer (the same range on both sides - buffers are
 * allocated full-frame on every rank, so a halo row lands at the address it has on its owner) moving between this rank and
 * `peer`. */
typedef struct HkTransfer {
  uint32_t buffer;   /* HkBuffer */
  uint32_t peer;     /* rank (= band index) on the other side */
  uint32_t is_recv;  /* 1: this rank receives rows `peer` owns; 0: this rank sends rows it owns */
  uint32_t _pad;
  uint64_t offset;   /* bytes from the start of the buffer */
  uint64_t bytes;
} HkTransfer;
/* Every transfer rank `rank` of `n_ranks` takes part in before `stage` (hk_band_plan_for's stage argument, including
 * HK_STAGE_TEMPORAL_WITH_HISTORY), sends AND receives, in ONE global order all ranks derive identically (the receive plans of
 * rank 0, 1, ... in turn) - the order a transport that pairs sends with receives by issue order (RCCL) needs.  Pure host
 * logic; out may be NULL to query the count. */
int hk_band_schedule(uint32_t width, uint32_t height, float upscale_ratio, uint32_t rank, uint32_t n_ranks, uint32_t stage,
                     uint32_t frame_number, const HkSettings* settings, HkTransfer* out, uint32_t* n_out);
int hk_band_schedule_bounds(uint32_t width, uint32_t height, float upscale_ratio, const uint32_t* bounds, uint32_t rank,
                            uint32_t n_ranks, uint32_t stage, uint32_t frame_number, const HkSettings* settings, HkTransfer* out,
                            uint32_t* n_out);
/* the schedule of hk_band_migration_plan (above: "Bands of equal MEASURED time") */
int hk_band_migration_schedule(uint32_t width, uint32_t height, float upscale_ratio, const uint32_t* old_bounds, const uint32_t* new_bounds, uint32_t rank,
                               uint32_t n_ranks, uint32_t next_frame_number, const HkSettings* settings, HkTransfer* out, uint32_t* n_out);
/* SURVEY 8e step 7, the gather of a finished image: the transfers of `rank` when band `root` collects every band's rows of
 * `buffer` (the root: one receive per other band, in band order; band r: one send).  Which rows of a buffer a band owns follows
 * the buffer's kind: render rows, two rows per render row for the SMAA Tu4x outputs, window rows for the FSR1 outputs.
 * upscale_kind: HkUpscaleKind of the settings the frame was rendered with; bounds: NULL = the equal split. */
int hk_band_gather_schedule(uint32_t width, uint32_t height, float upscale_ratio, uint32_t upscale_kind, const uint32_t* bounds,
                            uint32_t rank, uint32_t n_ranks, uint32_t root, uint32_t buffer, HkTransfer* out, uint32_t* n_out);
/* the image the overlay presents (overlay.rs:226-231) after a frame rendered with these settings and frame flags: the tone-mapped
 * image, or with HK_FRAME_ANTIALIAS the TAA / SMAA Tu4x / sharpened FSR1 output */
uint32_t hk_final_buffer(const HkSettings* settings, uint32_t frame_flags);

/* ------------------------------------------------------------------ halo exchange inside the boundary: one process per GPU, RCCL over xGMI */
/* The reference's LightNode / PostProcessNode record every dispatch of a frame into one command encoder (light.rs:590-702);
 * a sharded frame needs a neighbour exchange between the temporal and the spatial dispatches (light.rs:689-697) and before
 * the denoiser.  With a communicator attached, hk_frame_render performs those exchanges itself, on the context's stream:
 *   [exchange C, history rows]  TEMPORAL  exchange A  SPATIAL  exchange B  POST_PROCESS  [exchange D  ANTIALIAS  exchange E  UPSCALE]
 * as ncclSend / ncclRecv pairs inside one ncclGroupStart / ncclGroupEnd per exchange (librccl is loaded on first use; a
 * single-GPU host never touches it).  Rank 0 obtains the id, ships its HK_COMM_ID_BYTES bytes to the other ranks by any host
 * channel (a Bevy app: its own launcher; bench.py: the torch.distributed store), every rank calls hk_comm_init - which also
 * does hk_set_band(rank, n_ranks) - and then simply renders frames. */
#define HK_COMM_ID_BYTES 128
int hk_comm_unique_id(uint8_t id[HK_COMM_ID_BYTES]);
/* Pre-flight for the rendezvous: HK_OK iff librccl loads with every entry point the exchange uses and the context's device
 * can be made current.  ncclCommInitRank blocks until all n_ranks have called it, so a launcher first lets every rank
 * report this over its host channel and only calls hk_comm_init when ALL ranks passed - a rank that cannot bring RCCL up
 * then fails the job instead of leaving the healthy ranks waiting inside the rendezvous. */
int hk_comm_available(hk_ctx* ctx);
int hk_comm_init(hk_ctx* ctx, uint32_t rank, uint32_t n_ranks, const uint8_t id[HK_COMM_ID_BYTES]);
int hk_comm_destroy(hk_ctx* ctx);
/* rows of last frame's reservoirs / AA history fetched from the neighbours before TEMPORAL / ANTIALIAS (exchange C).  Since ABI 7
 * the default is HK_HISTORY_AUTO: hk_frame_begin derives the count from the frame's own uniforms, the scene's bounds and the
 * instances that moved (hk_history_rows_bound; 0 for a static view, so a static frame exchanges nothing).  An explicit count
 * overrides it (tests; hosts that know better).  hk_history_rows returns the count in force for the frame most recently begun.
 * hk_comm_set_history_rows is the ABI 6 name of hk_set_history_rows. */
#define HK_HISTORY_AUTO 0xFFFFu
int hk_set_history_rows(hk_ctx* ctx, uint32_t rows);
int hk_history_rows(hk_ctx* ctx, uint32_t* rows);
int hk_comm_set_history_rows(hk_ctx* ctx, uint32_t rows);
/* world bounds of the uploaded scene (the union of the instances' boxes; what hk_history_rows_bound takes) */
int hk_scene_bounds(hk_ctx* ctx, float min[3], float max[3]);
/* one exchange by hand (hosts that drive hk_frame_stage themselves): everything hk_band_schedule lists for `stage` */
int hk_comm_exchange(hk_ctx* ctx, uint32_t stage, const HkSettings* settings);
/* rank `root` collects every other rank's rows of `buffer` (hk_band_gather_schedule as ncclSend / ncclRecv in one group, on the
 * context's stream); hk_frame_render(.., HK_FRAME_GATHER) does it for hk_final_buffer with root 0 */
int hk_comm_gather(hk_ctx* ctx, uint32_t buffer, uint32_t root);

/* ------------------------------------------------------------------ one process, several GPUs (hk_create(n_gpus, device_ids)) */
/* Bevy renders from ONE process and one render thread: hk_multi is the same band-sharded frame driven by a single host
 * thread - n contexts, one per device, scene replicated, each rendering its band; halo rows move with hipMemcpyPeerAsync on
 * the receiver's stream, ordered against the owner's stream with events (no host synchronisation inside a frame).
 * device_ids may repeat (several bands on one GPU: how the path is tested where only one GPU exists). */
typedef struct hk_multi hk_multi;
int hk_multi_create(uint32_t n, const int* device_ids, uint32_t flags, hk_multi** out);
void hk_multi_destroy(hk_multi* m);
int hk_multi_context(hk_multi* m, uint32_t i, hk_ctx** out); /* the i-th band's context (borrowed) */
int hk_multi_upload_scene(hk_multi* m, const hk_scene_builder* b);
/* hk_load_scene for every band: the trees are built once (on band 0's device) and written back, the other bands take the finished builder */
int hk_multi_load_scene(hk_multi* m, hk_scene_builder* b, uint32_t tree_mode);
/* hk_add_meshes for every band: deferred trees are built once (on band 0's device) and written back, the other bands take the finished
 * builder's new ranges */
int hk_multi_add_meshes(hk_multi* m, hk_scene_builder* b, uint32_t tree_mode);
/* hk_remove_meshes on every band's context (each validates before it writes; the bands hold the same scene, so they agree) */
int hk_multi_remove_meshes(hk_multi* m, const HkMeshExtent* removed, uint32_t n);
int hk_multi_upload_scene_instances(hk_multi* m, const hk_scene_builder* b);
int hk_multi_refit_scene_instances(hk_multi* m, hk_scene_builder* b, uint32_t* moved); /* hk_refit_scene_instances on every band's replica */
int hk_multi_rebuild_scene_trees(hk_multi* m, uint32_t mode);
/* hk_update_mesh_vertices / hk_set_mesh_skin / hk_skin_mesh / hk_set_mesh_morph_targets / hk_deform_meshes on every band's replica */
int hk_multi_update_mesh_vertices(hk_multi* m, const HkMeshIndex* mesh, uint32_t n_vertices, const float* positions, const float* normals);
int hk_multi_set_mesh_skin(hk_multi* m, const HkMeshIndex* mesh, uint32_t n_vertices, const float* bind_positions, const float* bind_normals,
                           const uint16_t* joint_indices, const float* joint_weights);
int hk_multi_skin_mesh(hk_multi* m, const HkMeshIndex* mesh, const float* joint_matrices, uint32_t n_joints);
int hk_multi_set_mesh_morph_targets(hk_multi* m, const HkMeshIndex* mesh, uint32_t n_vertices, uint32_t n_targets, const float* base_positions,
                                    const float* base_normals, const float* position_deltas, const float* normal_deltas);
int hk_multi_deform_meshes(hk_multi* m, const HkMeshDeform* items, uint32_t n);
int hk_multi_rebuild_mesh_tree(hk_multi* m, const HkMeshIndex* mesh, uint32_t mode);
int hk_multi_set_mesh_motion_vectors(hk_multi* m, const HkMeshIndex* mesh, uint32_t enable);   /* every band's context; the bands' apron rows get the pass with their primary rays */
int hk_multi_set_band_bounds(hk_multi* m, const uint32_t* bounds, uint32_t n_bounds);
/* hk_migrate_bands for the one-process form: the rows that change owner travel as peer copies, then every band takes the new split */
int hk_multi_migrate_bands(hk_multi* m, const uint32_t* new_bounds, uint32_t n_bounds, uint32_t next_frame_number, const HkSettings* settings);
/* the root band's context collects every other band's rows of `buffer` on its own device (peer copies ordered by events, no host wait) */
int hk_multi_gather(hk_multi* m, uint32_t buffer, uint32_t root);  /* hk_set_band_bounds on every band's context */
int hk_multi_update_scene_instances(hk_multi* m, hk_scene_builder* b, uint32_t tree_mode);  /* hk_update_scene_instances on every band's replica */
int hk_multi_change_scene_instances(hk_multi* m, hk_scene_builder* b, const uint32_t* origins, uint32_t n, uint32_t tree_mode);  /* hk_change_scene_instances on every band's replica (the builder is finished once) */
int hk_multi_upload_textures(hk_multi* m, const HkImageDesc* images, uint32_t n_images);
/* hk_update_materials / hk_update_texture on every band's replica (an emitter switched on or off finishes the builder once) */
int hk_multi_update_materials(hk_multi* m, hk_scene_builder* b, uint32_t tree_mode, uint32_t* changed);
int hk_multi_update_texture(hk_multi* m, uint32_t index, const HkImageDesc* image);
int hk_multi_upload_noise(hk_multi* m, const uint8_t* rgba, size_t bytes);
int hk_multi_resize(hk_multi* m, uint32_t width, uint32_t height, float upscale_ratio);
int hk_multi_set_history_rows(hk_multi* m, uint32_t rows);
int hk_multi_frame_render(hk_multi* m, const HkFrame* frame, const HkView* view, const HkPreviousView* previous_view,
                          const HkLights* lights, const HkSettings* settings, uint32_t flags);
int hk_multi_wait(hk_multi* m);
/* the union of the bands: every band's own rows of `buffer` (a buffer whose rows are render rows, or full-size rows at
 * upscale ratio 1) gathered into one host image of the buffer's full size */
int hk_multi_read_buffer(hk_multi* m, uint32_t buffer, void* dst, size_t bytes);

/* ------------------------------------------------------------------ buffer access */
int hk_buffer_info(hk_ctx* ctx, uint32_t buffer, uint32_t* width, uint32_t* height, uint32_t* bytes_per_pixel);
/* synchronous copies (wait for the stream first).  Both position planes may be written: the library keeps the depths (.w) of
 * HK_BUF_POSITION and of HK_BUF_PREVIOUS_POSITION in planes of its own, which the denoiser and the anti-aliasing kernels gather
 * from, and copies them again from a plane hk_write_buffer wrote before the next dispatch that reads them (hk_pass_run and
 * hk_frame_stage alike).  A frame that writes neither launches nothing for it. */
int hk_read_buffer(hk_ctx* ctx, uint32_t buffer, void* dst, size_t bytes);
int hk_write_buffer(hk_ctx* ctx, uint32_t buffer, const void* src, size_t bytes);
/* raw device pointer for zero-copy views (a host that composites or exchanges the buffers itself).  *bytes = the size of the
 * ALLOCATION, which does not depend on the upscale kind in effect (hk_buffer_info gives the logical size); the pointer is
 * valid until the next hk_resize (and, for the double-buffered ids, names another plane after the next hk_frame_begin).
 * A host that WRITES a G-buffer, albedo, render or variance plane through such a pointer does so before the frame's first stage (with
 * HK_FRAME_EXTERNAL_GBUFFER for the G-buffer): between two hk_frame_stage calls of one frame the library may rely on what the stages
 * before wrote there (the empty-tile plane of the primary rays).  Asking for the pointer of one of those ids makes the frame in
 * progress and the next one take no such shortcut; a pointer kept for longer is the host's to use by this rule.
 * The library no longer rewrites what a plane already holds: where a tile had no geometry in the last frame of the same parity and has
 * none again, the G-buffer, albedo, render and variance planes keep the background's constants that frame stored.  So a host that
 * writes one of them (the PREVIOUS ids included) through a pointer it kept, outside a HK_FRAME_EXTERNAL_GBUFFER frame, asks for the
 * pointer again after writing, or uses hk_write_buffer: either makes the following frames store every pixel again.
 * The same holds for the planes the denoiser and tone mapping write - HK_BUF_DENOISE_INTERNAL0..3, HK_BUF_DENOISE_INTERNAL_VARIANCE,
 * HK_BUF_DENOISE_RENDER0..2, HK_BUF_TONE_MAPPED and HK_BUF_PREVIOUS_TONE_MAPPED: where a tile had no geometry in the frame before and
 * has none again (the tone-mapped image: in the last frame of the same parity as well) they keep the constants that frame stored.
 * hk_write_buffer into ANY plane, or asking for the pointer of one of these ids, makes the following frames store every pixel of
 * them again.
 * Asking for HK_BUF_PREVIOUS_POSITION makes the next anti-aliasing dispatch copy that plane's depths again (as after
 * hk_write_buffer); a host that writes it through a pointer it kept asks again after writing, or uses hk_write_buffer. */
int hk_device_ptr(hk_ctx* ctx, uint32_t buffer, void** ptr, size_t* bytes);
/* the HIP stream the context enqueues its frames on.  Without hk_set_stream it is the context's own; the context's FIRST frame may
 * create it again at the device's highest priority (round 6: the frame's dependent chain ahead of the direct-light and a-trous
 * dispatches of the other streams when frames are small) - so ask after that frame: a handle taken before it may name a stream that
 * no longer exists. */
int hk_stream(hk_ctx* ctx, void** hip_stream);
/* Enqueue all subsequent work on a HIP stream owned by the host (e.g. the stream its RCCL calls
 * are ordered against) instead of the context's own stream; NULL restores the context's stream. */
int hk_set_stream(hk_ctx* ctx, void* hip_stream);
/* bit i set = bracket every dispatch of HkPass i with HIP events (see HkStats) */
int hk_set_timing_mask(hk_ctx* ctx, uint32_t pass_mask);
int hk_get_stats(hk_ctx* ctx, HkStats* out);
int hk_reset_stats(hk_ctx* ctx);
/* Which schedule the indirect_lit_ambient dispatch of the frame most recently begun takes (see HK_CTX_WAVEFRONT): 0 = fused
 * kernel, 1 = wavefront (ray queues).  Depends on the flags, the frame's indirect_bounces and the size of the uploaded scene. */
int hk_indirect_schedule(hk_ctx* ctx, uint32_t* out);
/* How rays walk the scene currently uploaded (light.wgsl:400-486 is the reference walk):
 *   HK_TRAVERSAL_REFERENCE  the reference's two-level walk in the reference's node order - bit-exact; always with
 *                           HK_CTX_EXACT_TRAVERSAL, and for LDS-resident scenes whose instances do not share one transform
 *   HK_TRAVERSAL_THREADED   the two-level walk over eight direction-ordered flattenings (scenes beyond the LDS copy)
 *   HK_TRAVERSAL_ONE_LEVEL  ONE BVH over all triangles in the instances' shared local space (LDS-resident scenes whose
 *                           instances all have the same transform, e.g. the Cornell box): the reference's per-triangle
 *                           arithmetic on the reference's operands, so the closest hit is the reference's except where a
 *                           ray grazes an instance's world box within rounding or two candidates tie exactly.
 * orderings (may be NULL): how many direction orderings of the trees are stored (1, 2, 4 or 8).
 * HK_TRAVERSAL_WIDE is OR-ed into HK_TRAVERSAL_THREADED when the closest-hit walks take the wide records (HK_CTX_NO_WIDE_WALK). */
#define HK_TRAVERSAL_REFERENCE 0u
#define HK_TRAVERSAL_THREADED 1u
#define HK_TRAVERSAL_ONE_LEVEL 2u
#define HK_TRAVERSAL_WIDE 0x100u
int hk_traversal_mode(hk_ctx* ctx, uint32_t* out, uint32_t* orderings);

/* Test and measurement hooks (hk_debug_*, hk_measure_*) are declared in hikari_hip_debug.h: a host that renders binds none of them. */

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HIKARI_HIP_H */
