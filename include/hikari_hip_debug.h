/* hikari_hip_debug.h - test and measurement hooks of libhikari_hip.so.
 *
 * Not part of the drop-in boundary (include/hikari_hip.h is what a Bevy host binds): these entry points exist for the parity
 * tests (tests/), the benchmark's in-run ceilings (bench.py) and the profiling tools (tools/).  Same library, same C ABI rules. */
#ifndef HIKARI_HIP_DEBUG_H
#define HIKARI_HIP_DEBUG_H

#include "hikari_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* (exported next to the boundary's entry points; everything else in the library is hidden) */
#endif

/* Test hook: the instance tree (ordering 0) and the light tree as the device holds them, in the reference's HkNode layout. */
int hk_debug_read_trees(hk_ctx* ctx, HkNode* instance_nodes, uint32_t instance_cap, HkNode* emissive_nodes, uint32_t emissive_cap);
/* Test hook: the mesh-level node array as the device holds it - every ordering (1, or 8 for threaded scenes) of every mesh tree,
 * leaf boxes filled in and navigators folded, ordering-major, entry / exit words as stored - and the orderings count. */
int hk_debug_read_mesh_nodes(hk_ctx* ctx, HkNode* out, uint32_t cap, uint32_t* count, uint32_t* orderings);
/* Test hook: what the last hk_load_scene of this context did - out[0] meshes whose trees the device built, out[1] their triangles,
 * out[2] the kernel launches of that build (a library sort counted as one), out[3] pending meshes completed by the host instead. */
int hk_debug_last_load(hk_ctx* ctx, uint32_t out[4]);
/* Test hook: what the last hk_add_meshes of this context did - out[0] meshes whose trees the device built, out[1] their triangles, out[2]
 * the kernel launches of that build, out[3] meshes whose trees the host had built (laid out for their ranges), out[4] 1 if the scene
 * moved to a larger allocation.  All zero after a call that found nothing new. */
int hk_debug_last_add(hk_ctx* ctx, uint32_t out[5]);
/* Measurement hook (tools/add_mesh_probe.py): where the host time of the last hk_add_meshes went, in ms - out[0] the allocations of a
 * relocation (the larger scene, wide records, events), out[1] its copy launch and the switch of the scene pointers, out[2] the growth of
 * the context's mirrors, out[3] staging, host layout, the device build with its wait and the read-back.  Zero where a step did not run. */
int hk_debug_last_add_times(hk_ctx* ctx, double out[4]);
/* Test hook: what the last hk_add_meshes / hk_add_meshes_device of this context took from device memory - out[0] the sources, out[1] their
 * triangles, out[2] the kernel launches that assembled their records (phase 1: one, however many sources), out[3] the bytes of HkPrimitive
 * and HkVertex records the call staged host to device: those of the meshes the host added only (the full layout of a one-slot scene
 * uploads the whole mesh level again, and says so here).  hk_add_meshes leaves out[0..2] zero. */
int hk_debug_last_add_sources(hk_ctx* ctx, uint32_t out[4]);
/* Measurement hook (tools/mesh_source_probe.py): the last hk_add_meshes_device, in ms - out[0] the assembling launch between two HIP
 * events (only while HK_DEBUG_OPT_ADD_SOURCE_TIMES is set, else 0), out[1] the host's wait for the stream with the read-back of status and records, out[2] the builder's store. */
int hk_debug_last_add_source_times(hk_ctx* ctx, double out[3]);
/* Test hook: what the last hk_remove_meshes of this context did - out[0] meshes removed, out[1] their triangles, out[2] what the call enqueued,
 * counted where it is enqueued: kernel launches (the propagate of deformed boxes that goes first included) and the fill of the new rank
 * plane (it does not follow the number of meshes), out[3] the runs per plane (the surviving intervals), out[4] the path (0 the device
 * compaction, 1 the full layout on the host), out[5] the bytes the compaction launch moved.  All zero after a call with nothing to do. */
int hk_debug_last_remove(hk_ctx* ctx, uint64_t out[6]);
/* Measurement hook (tools/remove_mesh_probe.py): ms between two HIP events around the compaction launch of the last hk_remove_meshes
 * (waits for the launch; 0 for a call that took the full layout or had nothing to do) */
int hk_debug_last_remove_ms(hk_ctx* ctx, float* ms);
/* Measurement hook (tools/load_probe.py): where the host time of the last hk_load_scene went, in ms - out[0] host completion of meshes
 * beyond the device limit, out[1] the copy into the context's mirrors, out[2] layout of both regions and their upload, out[3] the device
 * build from its first launch to the end of the stream, out[4] the read-back, its unfolding and the write-back into the builder. */
int hk_debug_last_load_times(hk_ctx* ctx, double out[5]);
/* Test hook: one mesh as the device holds it after the pending deformations: the positions of the last deformation (of a mesh never
 * deformed on this context: gathered from the corners of its triangles, a vertex no triangle names zero; the box their extent) and the vertex-plane normals (4 floats per vertex), the triangle planes (12
 * floats per triangle: v0, v1, v2 as xyz + the vertex-index word) and the mesh box (min xyz, max xyz) decoded from its six words.
 * *n_vertices / *n_triangles receive the counts; all four arrays NULL asks for the counts alone.  Reads only. */
int hk_debug_read_mesh_geometry(hk_ctx* ctx, const HkMeshIndex* mesh, float* positions, float* normals, uint32_t vertex_cap, float* triangles,
                                uint32_t triangle_cap, float box[6], uint32_t* n_vertices, uint32_t* n_triangles);
/* Test hook: the emitter records (8 floats each: position xyz, radius, surface area, then instance, alias offset, alias count as u32
 * bits) and the alias table (probability, index bits) as the device holds them; *n_records / *n_alias receive the counts. */
int hk_debug_read_emitters(hk_ctx* ctx, float* records, uint32_t records_cap, uint32_t* n_records, float* alias, uint32_t alias_cap, uint32_t* n_alias);
/* Test hook: what the last hk_deform_meshes / hk_deform_meshes_device of this context did and what followed it - out[0] items, out[1]
 * their vertices, out[2] their triangles, out[3] what the call enqueued (kernel launches + asynchronous memsets and copies; stream waits
 * and event records not counted: five, six where an item recomputed its normals), out[4] the kernel launches of the last propagation of deformed meshes' boxes to the instance level (the flush in front of a
 * frame or a read, after single-mesh calls too), out[5] the kernel launches of the last derivation of wide records.  out[0..3] are zero
 * until a batch ran; a refused batch leaves them as they were. */
int hk_debug_last_deform(hk_ctx* ctx, uint32_t out[6]);
/* Motion vectors (hk_set_mesh_motion_vectors): out[0] launches of the motion pass in the frame whose primary rays were enqueued last,
 * out[1] the meshes live in it (deformed since the frame before), out[2] the pixels the pass rewrote - counted, one atomic per wave,
 * only while HK_DEBUG_OPT_MOTION_COUNT is set (the call then waits for the frame); 0 otherwise. */
int hk_debug_last_motion(hk_ctx* ctx, uint32_t out[3]);
/* What the last accepted hk_set_instance_transforms_device did: out[0] its kernel launches (the two pose kernels, the refit of the named
 * instances, of the named emitters, of the two trees; the slot copy of a two-slot scene and event records not counted), out[1] 1 if it
 * copied the builder's mesh boxes to the device (the first call for an instance list), else 0.  A refused call leaves them as they were. */
int hk_debug_last_pose(hk_ctx* ctx, uint32_t out[2]);
/* What the last accepted hk_change_scene_instances did: out[0] the kernel launches of its device path - the move of a scene whose spare
 * slot had no room, the staged copy of the laid-out level, the carry of the survivors' poses (only where the poses are the device's),
 * the derive pass, the emitters' pass, the refit of a single-leaf tree, the copy of the previous models of instances at motion - which do
 * not follow the number of instances or edits; the two tree builds (hk_rebuild_scene_trees' launches) and event records are not
 * counted.  out[1] the instances carried over, out[2] the new ones, out[3] bit 0: the scene moved to larger slots, bit 1: the mirrors
 * were current and the call took hk_update_scene_instances' path (out[0] is 0 then).  A refused call leaves them as they were. */
int hk_debug_last_instance_change(hk_ctx* ctx, uint32_t out[4]);
/* What the last accepted hk_update_textures_device did: out[0] its items, out[1] its kernel launches (event records not counted; a scene
 * laid out first because an hk_upload_textures was pending is not part of it), out[2] the texels it wrote, saturated at 2^32 - 1.  A
 * refused call, or one with n == 0, leaves them as they were. */
int hk_debug_last_texture_update(hk_ctx* ctx, uint32_t out[3]);

/* Measurement hook ("measure the empirical HBM ceiling with a device copy/triad kernel in the same run"): streams
 * three private arrays of `bytes_per_array` bytes (use >= 1 GiB: the 256 MB Infinity Cache must not hold them) `reps` times
 * on the context's stream and returns the sustained rates in GB/s (1e9), HIP events around the launches: copy a = b moves
 * 2 x bytes per pass, triad a = b + s * c moves 3 x bytes. */
int hk_measure_hbm(hk_ctx* ctx, size_t bytes_per_array, uint32_t reps, double* copy_gbs, double* triad_gbs);
/* Measurement hook for the OTHER roof of the ray kernels: the rate at which the chip issues wave64 VALU instructions, in
 * 1e9 wave-instructions per second, from a register-only kernel of eight independent v_fma_f32 chains per lane (64 x iters
 * instructions per wave) run with 1, 2, 4 and 8 waves resident per SIMD (ginstr_s[0..3]).  One wave alone issues about one
 * instruction per 6 cycles; the ceiling (one per ~2 cycles per SIMD) needs four or more waves per SIMD. */
int hk_measure_valu(hk_ctx* ctx, uint32_t iters, double ginstr_s[4]);

/* Test hook: evaluate one of the library's device math routines elementwise (op: 0 sin, 1 cos,
 * 2 exp, 3 exp2, 4 log2, 5 pow(x, y), 6 min(x,y), 7 max(x,y), 8 f32->f16->f32, 9 x/y, 10 sqrt,
 * 11 saturate(x), 12 clamp(x, -1, 1), 13 saturate(x*y), 14 / 15 / 20 the unorm16 / snorm8 / unorm8 decode of the integer x;
 * 21 / 22 the sine / cosine of sincos_, 23 exp_nonpositive_, 24 quotient_by_reciprocal(x, 1.0 / (double)y), 25 the denoiser's
 * weight exp_nonpositive_(quotient_by_reciprocal(-|x|, 1.0 / (double)y)), 26 pow2_, 27 pow5_, 28 pow16_, 29 pow_quarter_,
 * 30 f32->f16->f32 of the f32 product x*y, 31 unorm16(x) and 32 snorm8(x) (the code, as a float: exact), 33 f32_to_u32(x) and
 * 34 f32_to_i32(x) (the 32 result bits, returned AS the bits of the float: read them back with a bit cast)).
 * x, y, out are HOST arrays of n floats, one result per item.
 * Ops 16..19 and 35..52 read SIXTEEN floats of x per item (x holds 16 n floats, q = x + 16 i):
 * 16 / 17 / 18 shading().rgb and 19 env_brdf().r for V = q[0..2], N = q[3..5], L = q[6..8] (each normalised first), base colour
 * q[9..11], radiance q[12..15] and the perceptual roughness y; 35 dot(q[0..2], q[3..5]), 36 dot(q[0..3], q[4..7]),
 * 37 / 38 / 39 cross(q[0..2], q[3..5]).xyz, 40 / 41 / 42 normalize(q[0..2]).xyz, 43 / 44 / 45 (mat3 of columns q[0..2], q[3..5],
 * q[6..8]) * q[9..11] .xyz, 46 / 47 / 48 / 49 (4x4 of columns q[0..3] .. q[12..15]) * v .xyzw where v is FOUR floats of y per
 * item (y holds 4 n floats and is required), 50 length(q[0..2]), 51 mix(q[0], q[1], q[2]), 52 fract(q[0]). */
int hk_debug_math(hk_ctx* ctx, uint32_t op, const float* x, const float* y, float* out, size_t n);

/* Measurement hook for the roof of the BVH walks of scenes beyond the LDS copy (round 4): every lane of
 * `waves_per_simd` resident waves per SIMD follows its own chain of `steps` DEPENDENT loads through a random permutation cycle over
 * `footprint_bytes` of records - `bytes_per_step` = 16 (one 16-B load per step), 32 (the two adjacent 16-B loads of a node step), 64 (a reservoir record) 128 (a record of the wide walk: eight adjacent 16-B loads, one 128-B line) or 129 (the same 128-B records fetched COOPERATIVELY: eight consecutive lanes load the eight pieces of one lane's record - round 5 experiment) -
 * i.e. 64 unrelated addresses per wave-level load instruction and no reuse.  Returns the rate of wave-level load instructions
 * (1e9 / s) and of loaded bytes (lanes x bytes_per_step per step; GB/s).  No walk of that shape runs faster on the chip: the
 * trace kernels of configs 3 / 4 are priced against it in bench.py (the HBM roof is meaningless for them - they move little). */
int hk_measure_gather(hk_ctx* ctx, size_t footprint_bytes, uint32_t bytes_per_step, uint32_t waves_per_simd, uint32_t steps,
                      uint32_t workgroups /* 0 = CUs x waves_per_simd (the whole chip); else that many 256-thread workgroups */, double* gloads_s, double* gbytes_s);

/* Profiling hook (tools/wf_timeline.py): with HK_DEBUG_OPT_WF_TIMELINE set the trace stages of the queue-based indirect pass
 * run an instrumented twin that records, per stage, when the ray queue ran dry, when the last persistent wave left and how long
 * the rays' walks were (hk_kernels.hpp WfBuffers::timeline: 64 stages x 32 u64, wall_clock64 ticks of 10 ns). */
int hk_debug_read_wf_timeline(hk_ctx* ctx, unsigned long long* out, uint32_t n /* 64 * 32 */);

/* Test hook for the RCCL data path on a box with ONE GPU (RCCL refuses two ranks on one device, so no halo exchange between
 * ranks can run there): rows [row_begin, row_end) of `src_buffer` travel to the same rows of `dst_buffer` (same shape) of the
 * SAME context as an ncclSend to the context's own rank paired with an ncclRecv from it, inside one ncclGroupStart / ncclGroupEnd,
 * ordered against the context's stream - the very function (comm.cpp run_transfers) hk_frame_render's exchanges and hk_comm_gather go
 * through.  Needs hk_comm_init (a communicator of any size; 1 rank on a one-GPU box). */
int hk_debug_comm_loopback(hk_ctx* ctx, uint32_t src_buffer, uint32_t dst_buffer, uint32_t row_begin, uint32_t row_end,
                           uint32_t mode /* 0: in stream order, like a halo exchange (lane 0); 2: the same on lane 1 (exchange B's); 1: overlapped with what follows, like the gather of a finished
                                            frame (hk_frame_render with HK_FRAME_GATHER) - complete before the frame of the same parity begins or
                                            anybody reads a buffer */);

/* Test hook (round 5): how many spatial_reuse launches of this context took the WINDOWED form of the kernel (the depths its taps reach
 * and the lists of surviving taps in LDS: kernels.hip) since hk_create.  Which form a launch takes: by its size, or what
 * hk_debug_set_option(HK_DEBUG_OPT_SPATIAL_WINDOW) says. */
int hk_debug_spatial_windowed_launches(hk_ctx* ctx, uint64_t* out);
/* ... and how many spatial_reuse launches were handed the table of the background's known records (kernels.hip k_spatial_known_fill: the
 * re-pack of the two records the temporal passes store to a background pixel, computed once per context) since hk_create: every one
 * while HK_DEBUG_OPT_SPATIAL_KNOWN is on, none while it is off. */
int hk_debug_spatial_known_launches(hk_ctx* ctx, uint64_t* out);

/* Test hook (round 6): the priority the context's own main stream was created at - 0 the default, 1 the device's highest, and whether the
 * rule has decided yet (bit 1: it decides at the context's first frame; hk_debug_set_option(HK_DEBUG_OPT_MAIN_PRIORITY) decides at once);
 * bit 2: the context has its fourth stream (the primary rays'), bits 8..27: frames whose primary rays were pipelined so far. */
int hk_debug_main_stream_priority(hk_ctx* ctx, uint32_t* out);

/* Test hook (round 6): 2 when the context's communicator has its second lane - a communicator (ncclCommSplit of the first) and a stream of
 * its own for what a band's POST-PROCESSING and the overlay wait for (exchange B, the gather, exchanges D / E), so that frame n's
 * exchange B and gather do not sit in front of frame n + 1's exchange A on one in-order queue - 1 when the library could not split. */
int hk_debug_comm_lanes(hk_ctx* ctx, uint32_t* lanes);

/* Switches for tests and A/B tools (round 6: the library itself reads NO environment variable).  Waits for the context's work, sets
 * the option, returns; options that change the scene layout take effect with the next frame. */
#define HK_DEBUG_OPT_SPATIAL_WINDOW 0u  /* which form of k_spatial_reuse a launch takes: -1 by its size (default), 0 plain, 1 windowed */
#define HK_DEBUG_OPT_FRAME_PIPELINE 1u  /* 0: the a-trous levels of frame n are NOT run beside frame n + 1's light passes (default 1) */
#define HK_DEBUG_OPT_WF_TIMELINE 2u     /* 1: the instrumented twin of the trace kernels (hk_debug_read_wf_timeline) */
#define HK_DEBUG_OPT_FLAT_WALK 3u       /* 0: no one-level tree for LDS scenes under one transform - they keep the reference's two-level walk (default 1) */
#define HK_DEBUG_OPT_FLAT_ORDERINGS 4u  /* 1..8 direction orderings of that tree (default 0: as many as keep it within 4 KB) */
#define HK_DEBUG_OPT_TRACE_UPDATE 5u    /* 1: timings of scene updates on stderr */
/* 6, 7 and 8 belonged to retired options and are not reused: hk_debug_set_option rejects them (HK_E_INVALID) */
#define HK_DEBUG_OPT_MAIN_PRIORITY 9u /* the priority of the context's own main stream, created again at once: -1 by the library's rule (the highest if the context dispatches at most 6 Mi pixels per frame; what the context's first frame decides by itself), 0 the default priority, 1 the highest.  A/B and tests: a stream created again several times ends up sharing a hardware queue */
#define HK_DEBUG_OPT_PREPASS_PIPELINE 10u /* a frame's primary rays on a stream of their own beside the previous frame's spatial pass, where the order allows (context.hip stage TEMPORAL): -1 by the library's rule (default: scenes beyond the LDS copy in frames of up to 3 Mi pixels, on a context whose chain runs at the highest priority), 0 never, 1 whenever the order allows */
#define HK_DEBUG_OPT_LOAD_DEVICE_LIMIT 12u /* hk_load_scene completes a deferred mesh of more than this many triangles on the host instead of the device (default 0: HK_MESH_REBUILD_MAX_TRIANGLES); tests reach that path without a mesh of four million triangles */
#define HK_DEBUG_OPT_MESH_REBUILD_ONE_WORKGROUP 11u /* 1: hk_rebuild_mesh_tree (HK_TREE_SAH) runs the top levels of its build in one workgroup at any mesh size, as the instance tree's build does (default 0: on the whole chip from 32 768 triangles); the same tree either way - the A/B of tools/deform_probe.py */
#define HK_DEBUG_OPT_KNOWN_RESULTS 13u /* 0: no launch is handed the empty-tile plane of the frame's primary rays - every wave computes its way to the background constants, and stores them whatever the planes hold (default 1; the A/B, tests/test_known_results_gpu.py and tests/test_background_stores_gpu.py) */
#define HK_DEBUG_OPT_ADD_SOURCE_TIMES 16u /* 1: hk_add_meshes_device records two timed events around its assembling launch (hk_debug_last_add_source_times out[0]; default 0: a product call makes and records none) */
#define HK_DEBUG_OPT_MOTION_COUNT 15u /* 1: the motion pass counts the pixels it rewrites (hk_debug_last_motion; default 0) */
#define HK_DEBUG_OPT_SPATIAL_KNOWN 14u /* 0: no spatial_reuse launch is handed the table of the background's known records - every background wave loads, unpacks and re-packs its input - and the windowed form of the kernel is handed no empty-tile / kept-tile plane (default 1; the A/B and tests/test_spatial_background_gpu.py) */
int hk_debug_set_option(hk_ctx* ctx, uint32_t option, int64_t value);
/* Test hook of the empty-tile plane (one byte per 8x8 tile of the render image, row-major, (w + 7) / 8 x (h + 7) / 8; 1 = every primary
 * ray of the tile missed): waits for the context's work, copies the plane of the current frame parity into out_bytes (n = the number of
 * tiles, HK_E_INVALID otherwise) and returns in *launches_given_the_plane how many kernel launches of hk_frame_stage were handed a plane
 * since the context was created.  A frame whose primary rays did not write the plane (HK_DEBUG_OPT_KNOWN_RESULTS 0, an upscale ratio
 * other than 1, bands, a host-rasterised G-buffer, the frame after hk_write_buffer) leaves the bytes as they were and adds no launch. */
int hk_debug_empty_tiles(hk_ctx* ctx, uint8_t* out_bytes, size_t n, uint64_t* launches_given_the_plane);
/* hk_multi_*: 1 = the calling thread enqueues every band's launches one after another instead of one thread per band (process-wide) */
int hk_debug_multi_serial(int on);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
