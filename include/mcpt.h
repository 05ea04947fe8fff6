/* mcpt.h — C ABI of the MI355X path tracer (libmcpt.so).
 *
 * Drop-in boundary for the reference's hot path.  Two halves:
 *
 *  1. Device renderer — replaces the GL program `prg_ray` (raytracer.vert +
 *     raytracer_func.frag + tp/<variant>.frag + main.frag), its texture/uniform ABI
 *     and the additive RGB32F FBO of MontecarloGPU/montecarlo.cpp:384-386, 408-477.
 *  2. Host scene producer — replaces ScenePrimitives / BVH_KDtree / BVH_GPU_Scene
 *     (bvh_gpu/scene.h:75-185, bvh.h:10-60, gpu_bvh_scene.h:35-121) and the canonical
 *     camera (easycppogl/camera.cpp:53-95 + montecarlo.cpp:388-389, 404-405, 439-440).
 *
 * Conventions: plain pointers and sizes, no torch types.  Matrices are 16 floats,
 * column-major (GL / Eigen storage).  Images are H rows × W pixels × RGB f32, row 0 =
 * bottom (GL window coordinates).  Every function returns an int status: 0 = ok,
 * negative = error (see mcpt_status); mcpt_error_string() describes it.  The caller
 * owns host arrays; the library owns device copies.  One context per GPU; calls on
 * one context are not thread-safe; contexts on different GPUs may run concurrently.
 * There is NO CPU fallback: every render call runs the HIP kernel or fails.
 */
#ifndef MCPT_H_
#define MCPT_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum mcpt_status {
  MCPT_OK = 0,
  MCPT_ERR_INVALID_ARG = -1,
  MCPT_ERR_NO_SCENE = -2,
  MCPT_ERR_NO_TARGET = -3,
  MCPT_ERR_HIP = -4,         /* a HIP runtime call failed (no GPU, launch failure ...) */
  MCPT_ERR_NOT_FINALIZED = -5,
  MCPT_ERR_BAD_SCENE = -6,
  MCPT_ERR_NO_GUIDES = -7,   /* mcpt_denoise / mcpt_read_guides without current guide buffers */
  MCPT_ERR_NO_STATS = -8,    /* a statistics query with statistics off, fewer than two batches or no error map */
  MCPT_ERR_NO_ADAPTIVE = -9, /* an adaptive-sampling call with the adaptive mode off (mcpt_adaptive_begin) */
  MCPT_ERR_NO_TEMPORAL = -10, /* a temporal call with the temporal mode off (mcpt_temporal_begin) */
};

/* integrator variants: the SrcLoader list of MontecarloGPU/montecarlo.cpp:27 */
enum mcpt_variant {
  MCPT_MONTECARLO = 0,       /* tp/montecarlo.frag        */
  MCPT_MAT = 1,              /* tp/montecarlo_mat.frag    */
  MCPT_MAT_TR = 2,           /* tp/montecarlo_mat_tr.frag */
};

/* BVH traversal strategy of the kernel (same results, different speed) */
enum mcpt_traversal {
  MCPT_TRAVERSAL_AUTO = 0,   /* measured: after a scene upload, launches of >= 2^24 samples time
                                the schedule candidates twice each (per-lane walks with 1/2/4 pass
                                segments per work item, the wave-coherent walk for BVH depth < 8,
                                the deep-BVH knobs at 4/8 segments for depth >= 8; never the stream
                                schedule); later launches of that shape use the fastest */
  MCPT_TRAVERSAL_LANE = 1,   /* each lane walks its own DFS (divergent, vector loads) */
  MCPT_TRAVERSAL_WAVE = 2,   /* the wave walks the union of its lanes' DFS orders (scalar loads) */
  MCPT_TRAVERSAL_STREAM = 3, /* wavefront schedule: a pool of path slots in HBM, iterations of one
                                trace kernel (persistent waves, a lane takes the next queued ray as
                                soon as its walk ends) and one shade kernel.
                                Variant montecarlo.frag, scenes without meshes, bounces > 0; other
                                renders run the per-lane walk.  mcpt_render returns once the
                                iterations have been issued (it waits on the device while it issues
                                them, to know when the slots are done).  Only when selected: AUTO
                                never times it (5 % behind the megakernel on the deepest BVH) */
};

/* algorithmic-byte event counters, index order */
enum mcpt_event {
  MCPT_EV_NODE = 0, MCPT_EV_LEAF, MCPT_EV_PRIM, MCPT_EV_CAND, MCPT_EV_GEOM, MCPT_EV_COLMAT,
  MCPT_EV_SAMPLE, MCPT_EV_TRAV, MCPT_EV_MESH, MCPT_EV_TRI, MCPT_EV_MGEOM, MCPT_EV_COUNT
};

typedef struct mcpt_ctx mcpt_ctx;
typedef struct mcpt_scene mcpt_scene;

const char* mcpt_error_string(int status);
int mcpt_version(void);
/* Which diagnostic build this library is (never a timed build): bit MCPT_BUILD_CHECKED the
 * bounds-checked build (make checked: out-of-range work-item / split / segment indices are counted
 * and skipped, every sub-launch is waited for and a fault or count fails the render call with the
 * sub-launch named), MCPT_BUILD_STAMPS / _LANESTATS / _BLOCKTIMES the instrumented builds,
 * MCPT_BUILD_DRIVER_MATH a GL-driver-arithmetic build.  0: the shipped library. */
enum { MCPT_BUILD_CHECKED = 1, MCPT_BUILD_STAMPS = 2, MCPT_BUILD_LANESTATS = 4, MCPT_BUILD_BLOCKTIMES = 8,
       MCPT_BUILD_DRIVER_MATH = 16 };
int mcpt_build_flags(void);

/* ---------------------------------------------------------------------------------
 * 1. device renderer
 * --------------------------------------------------------------------------------- */

/* create a context on HIP device `device_ordinal` (replaces GLViewer ctx + prg_ray) */
int mcpt_create(int device_ordinal, mcpt_ctx** out);
int mcpt_destroy(mcpt_ctx* ctx);

/* Upload a finalized scene in the reference's texture layouts:
 *   prims  : n_prims × 64 f32 (16 RGBA texels per PrimData, scene.h:64-73)
 *   nodes  : (2^(depth+1)-1) × 6 f32 (bbmin.xyz, bbmax.xyz)  — tex_bb, gpu_bvh_scene.cpp:39-41
 *   leaves : 2^depth i32 (prim index or -1)                   — tex_ind, gpu_bvh_scene.cpp:143-144
 * Replaces BVH_GPU_Scene::finalize's Texture2D uploads (gpu_bvh_scene.cpp:143-160) and
 * the uniforms nb_prims(1), bvh_depth(2), nb_emissives(20).  Transforms must be affine
 * (row 3 = 0,0,0,1: the shader only uses .xyz).  Limit: n_prims < 2^24 (MCPT_ERR_INVALID_ARG
 * otherwise) — the kernel packs a hit's primitive index, shape and face into one 32-bit word
 * (shape << 28 | face << 24 | index), which keeps the walk's hit record in 7 registers.
 * Synchronous. */
int mcpt_upload_scene(mcpt_ctx* ctx, const float* prims, int n_prims, const float* nodes,
                      const int* leaves, int depth, int nb_emissives);

/* Upload the scene's meshes (replaces the tex_tri_/tex_p_/tex_n_ textures and the per-mesh
 * BVH rows of tex_bb_/tex_ind_, gpu_bvh_scene.cpp:87-118, 160-186).  Layouts: see
 * mcpt_scene_get_mesh_buffers.  n_meshes = 0 removes them.  Call after mcpt_upload_scene;
 * a CODE_MESH primitive's record holds its mesh id (texel 12 .y, "mesh_line").  Limits (else
 * MCPT_ERR_BAD_SCENE): BVH depth <= 24 per mesh, and the device's mesh BVH records (64 B per
 * internal node + 64 B per leaf, all meshes) within 4 GiB — the walk addresses them by 32-bit
 * offsets — i.e. about 33 M triangles in all. */
int mcpt_upload_meshes(mcpt_ctx* ctx, int n_meshes, const int* info, int n_nodes, const float* nodes, int n_leaves,
                       const int* leaves, int n_tris, const int* tris, int n_verts, const float* verts,
                       const float* normals);

/* Deforming meshes (no reference equivalent: its meshes are static): new vertices
 * into the uploaded meshes, then a refit of their BVH records on the device — same topology (the
 * triangles, the depth and the leaf order of the upload), new boxes.
 *
 * mcpt_update_mesh_vertices copies n_vertices x 3 f32 positions and normals from the host (through a
 * staging buffer of the context) over the uploaded vertices first_vertex .. (indices into the flat
 * verts / normals arrays of mcpt_upload_meshes: mcpt_scene_mesh_vertex_range);
 * mcpt_update_mesh_vertices_device takes them packed in memory of the context's device, complete
 * before the call (a simulation's output).  One kernel on the context's stream widens them into
 * place.  MCPT_ERR_BAD_SCENE with no meshes uploaded, MCPT_ERR_INVALID_ARG for a range outside the
 * uploaded vertices.  The caller keeps every vertex inside the Mesh::BB() its mesh was added with
 * (mcpt_scene_update_mesh checks that on the host): the instances' scene-level boxes do not move.
 *
 * mcpt_refit_mesh rewrites mesh mesh_id's (-1: every mesh's) leaf triangle records and child-pair
 * records from the current vertices: the bits mcpt_upload_meshes writes from the buffers of a
 * mcpt_scene_update_mesh with the same vertices.  It runs on the context's stream behind every
 * queued render and ahead of every later one, without a host wait unless `out` is given (then it
 * waits once and fills the record).  Both calls invalidate the guide buffers and empty the
 * temporal history, as mcpt_upload_meshes does; the AUTO schedule, the work-item order, the noise
 * statistics, the adaptive state and the accumulator stay (whether to clear them is the caller's
 * decision).  A mesh of depth 0 (one triangle) has no records: only its vertices change.
 * MCPT_ERR_BAD_SCENE with no meshes uploaded, or for a mesh uploaded with a leaf pair that holds no
 * triangle (mcpt_scene_add_mesh never builds one); MCPT_ERR_INVALID_ARG for an unknown mesh id; the
 * records stay as they are then. */
typedef struct mcpt_refit_t {
  long long triangles;        /* leaf triangle records written */
  long long leaves;           /* leaves visited (2^depth per mesh) */
  long long internal_nodes;   /* child-pair records written */
  float device_ms;            /* the refit's kernels, from HIP events */
  int has_root;               /* 1: root_box is set (a single mesh of depth >= 1) */
  float root_box[6];          /* the mesh's new root box (min.xyz, max.xyz), mesh space */
} mcpt_refit_t;
int mcpt_update_mesh_vertices(mcpt_ctx* ctx, int first_vertex, int n_vertices, const float* verts, const float* normals);
int mcpt_update_mesh_vertices_device(mcpt_ctx* ctx, int first_vertex, int n_vertices, const void* verts_dev,
                                     const void* normals_dev);
int mcpt_refit_mesh(mcpt_ctx* ctx, int mesh_id, mcpt_refit_t* out);
/* Rebuild of the uploaded mesh mesh_id's BVH on the device: a new leaf order from
 * the current vertices by segmented stable radix sorts of the triangle centres (depth - 1 rounds),
 * the triangle ids into the leaf records, then mcpt_refit_mesh's stages — the bits
 * mcpt_upload_meshes writes from the buffers of a mcpt_scene_rebuild_mesh with the same vertices
 * and triangles.  mesh_id == -1: every mesh, and only with tris == NULL.  tris: n_tris x 3
 * mesh-local vertex indices that replace the mesh's triangle rows first (n_tris must be the mesh's
 * count, every index below its vertex count, else MCPT_ERR_INVALID_ARG).  The flat arrays of
 * mcpt_upload_meshes do not say where a mesh's vertices begin: mcpt_set_mesh_vertex_counts gives the
 * context each mesh's vertex count, in mesh order (mcpt_scene_mesh_vertex_range; the counts add up
 * to the uploaded vertices and every mesh's triangles lie inside its range, else
 * MCPT_ERR_INVALID_ARG), once after an upload; without it a rebuild with tris is MCPT_ERR_BAD_SCENE
 * (the Python and C++ upload_scene make the call).  Ordering, state and refusals are
 * mcpt_refit_mesh's: the context's stream behind every queued render, no host wait unless `out` is
 * given, guides invalid and temporal history emptied, everything else kept; MCPT_ERR_BAD_SCENE with
 * no meshes, for a mesh uploaded with an all-empty leaf pair or with a depth other than
 * ceil(log2(triangles)); MCPT_ERR_INVALID_ARG for an unknown id; the records and triangles stay
 * as they are then.  A mesh of depth 0 has no order: with tris only its triangle row changes. */
typedef struct mcpt_rebuild_t {
  long long triangles;        /* triangles sorted (meshes of depth >= 2) */
  int rounds;                 /* segmented sort rounds run (depth - 1 per mesh) */
  int sort_passes;            /* radix passes launched (8 bits each) */
  float sort_ms;              /* triangle rows, centres, the sort and the leaf ids, from HIP events */
  float refit_ms;             /* the refit stages, from HIP events */
  int has_root;               /* 1: root_box is set (a single mesh of depth >= 1) */
  float root_box[6];          /* the mesh's new root box (min.xyz, max.xyz), mesh space */
} mcpt_rebuild_t;
int mcpt_rebuild_mesh(mcpt_ctx* ctx, int mesh_id, const int* tris, int n_tris, mcpt_rebuild_t* out);
int mcpt_set_mesh_vertex_counts(mcpt_ctx* ctx, int n_meshes, const int* counts);
/* Diagnostics: the device's mesh BVH records as they stand — the child-pair slots (4 x 4 f32 per
 * slot: (c_left, has) (w_left, in_range) (c_right, has) (w_right, 0); each mesh's run starts at an
 * even slot, internal node i at slot i + 1 of the run) and the leaf triangle records (4 x 4 f32 per
 * leaf: (A, triangle id bits) (B - A, 0) (C - A, 0) (0)).  mcpt_debug_mesh_record_sizes gives the
 * float counts the copy expects; a NULL pointer skips that array.  Synchronizes. */
int mcpt_debug_mesh_record_sizes(mcpt_ctx* ctx, size_t* pair_floats, size_t* leaf_floats);
int mcpt_debug_mesh_records(mcpt_ctx* ctx, float* pairs_out, size_t pair_floats, float* leaves_out, size_t leaf_floats);

/* uniform flat_face (raytracer_func.frag:26, location 3): flat triangle normals instead of
 * the area-weighted vertex normals.  The reference never sets it (false); default 0. */
int mcpt_set_flat_face(mcpt_ctx* ctx, int flat_face);

/* Set the framebuffer (replaces FBO RGB32F + resize_ogl, montecarlo.cpp:384-386, 616-626).
 * Row-band sharding for multi-GPU: this context renders global rows y whose band
 * (y / band_rows) satisfies band % world == rank; its accumulator holds only those
 * "local" rows, in increasing y.  Single GPU: band_rows = any > 0, world = 1, rank = 0.
 * Allocates and zeroes the accumulator; pass count reset to 0.  MCPT_ERR_INVALID_ARG when this
 * context's local rows × W reach 2^31 pixels (the kernels index a shard with 32-bit ints). */
int mcpt_set_target(mcpt_ctx* ctx, int W, int H, int band_rows, int world, int rank);
int mcpt_local_rows(mcpt_ctx* ctx, int* n_local_rows);
/* Explicit shard: this context renders the n_rows global rows rows[0..n_rows) (distinct, in
 * [0, H)), local row i = global row rows[i]; the accumulator holds n_rows × W pixels.
 * Results per pixel do not depend on the partition. */
int mcpt_set_target_rows(mcpt_ctx* ctx, int W, int H, const int* rows, int n_rows);
/* The balanced multi-GPU partition: bands of band_rows rows dealt to ranks
 * period by period with a rotation (period j: rank r takes band j·world + (r+j) mod world),
 * the rows after the last whole period dealt singly; every rank gets floor(H/world) or
 * ceil(H/world) rows.  Writes rank's rows (increasing; rows_out may be NULL to query the
 * count) and their number.  Host-only (no device). */
int mcpt_balanced_rows(int H, int world, int rank, int band_rows, int* rows_out, int* n_out);
/* The context's global row ids of its local rows (n_local_rows ints). */
int mcpt_local_row_ids(mcpt_ctx* ctx, int* rows_out);

/* Accumulate passes first_pass .. first_pass+n_passes-1 into the accumulator (the
 * glDrawArrays loop of montecarlo.cpp:454-466 with blend ONE/ONE).  Summation order
 * (DESIGN.md §3.3): per pixel, passes are summed from 0 within each chunk of 32
 * consecutive absolute pass numbers ((pass-1)/32), and chunk sums are added to the
 * accumulator in chunk order — results are identical for any GPU count and for any
 * split of a pass range into calls at multiples of 32.  Uniform ABI:
 * invPV(10), invV(6), numero_pass(4) = pass index, date(5), NB_BOUNCES(21),
 * refract_ind(24); variant = tp/ shader.  Asynchronous on the context's stream.
 * Scheduling (never the bits): a launch of >= 4,096 work items times its items
 * and the next launch of the same shape runs them costliest first (a device sort on the
 * context's stream: no host wait; env MCPT_ITEM_ORDER=0 turns it off); launches whose work items
 * hold several pass segments run the last workgroup-generation of that order one segment per
 * workgroup (env MCPT_TAIL_PIECES=0 turns that off); in mesh scenes, launches of whole 32-pass
 * chunks also run their costliest items in 4 pass ranges side by side (env MCPT_SPLIT_ITEMS=0
 * turns that off).  Device memory for it: 20 B per work item, and 100 MB of per-pass values
 * once a mesh launch splits items. */
int mcpt_render(mcpt_ctx* ctx, const float* invPV, const float* invV, int first_pass,
                int n_passes, float date, int bounces, float refract_ind, int variant);

/* Same, with the counting build of the kernel: adds MCPT_EV_COUNT event totals into
 * events[] (algorithmic bytes = Σ events × mcpt_event_bytes).  Synchronous. */
int mcpt_render_counted(mcpt_ctx* ctx, const float* invPV, const float* invV, int first_pass,
                        int n_passes, float date, int bounces, float refract_ind, int variant,
                        unsigned long long* events);
int mcpt_event_bytes(int event);

#define MCPT_DEBUG_SLOTS 64
/* Diagnostics: read the first min(n_slots, MCPT_DEBUG_SLOTS) of the context's device counter
 * slots into `out` (which holds n_slots values; the first MCPT_EV_COUNT are the event counters)
 * and optionally zero them all.  The counting launches and diagnostic builds (-DMCPT_STAMPS:
 * wave-cycle section totals; -DMCPT_LANESTATS) write them; slot 63 holds how many work items
 * the last work-item sort of a mesh scene's launch chose to split.  Synchronizes the
 * context's stream.  (Version 2: the n_slots argument; version 1 copied MCPT_DEBUG_SLOTS
 * values, 16 before round 4, whatever the caller's buffer held.) */
int mcpt_debug_counters(mcpt_ctx* ctx, unsigned long long* out, int n_slots, int reset);

/* Copy the local accumulator (n_local_rows × W × 3 f32) to the host and report the
 * number of passes accumulated (the caller divides: fs_frag, montecarlo.cpp:59-70).
 * Synchronizes the context's stream. */
int mcpt_read_accum(mcpt_ctx* ctx, float* rgb_out, int* pass_count);
int mcpt_clear_accum(mcpt_ctx* ctx);
/* The inverse of mcpt_read_accum: load n_local_rows × W × 3 f32 sums and the number of passes
 * they hold into the context's accumulator; later renders add to them (resuming a progressive
 * render from a checkpoint, mcpt_checkpoint_read).  Synchronizes the context's stream. */
int mcpt_write_accum(mcpt_ctx* ctx, const float* rgb, int pass_count);

/* Device pointer of the local accumulator (for an RCCL gather by the caller). */
int mcpt_accum_device_ptr(mcpt_ctx* ctx, void** dev_ptr, size_t* bytes);
/* Device-to-device copy of the local accumulator into a caller buffer of >= bytes
 * (e.g. a torch tensor that feeds the RCCL gather), ordered on the context's stream. */
int mcpt_copy_accum_device(mcpt_ctx* ctx, void* dst_dev_ptr, size_t bytes);

/* Multi-GPU frame assembly inside ONE process (the C++ host's N-GPU path: one context and
 * host thread per device): copy every shard context's local rows into `frame`'s accumulator
 * at their global rows, device to device (hipMemcpyPeerAsync over xGMI, one copy per run of
 * consecutive global rows), ordered after the shards' queued renders and on `frame`'s stream;
 * each shard's stream in turn waits for the copies that read its accumulator, so a
 * progressive caller may render into a shard again right after the call (its next passes
 * cannot reach rows still being copied).
 * `frame` holds a full-frame target of the shards' W x H (mcpt_set_target(W, H, b, 1, 0));
 * rows no shard holds keep their values; every shard must hold the same pass count, which
 * becomes frame's.  Replaces montecarlo.cpp's single-FBO read (:59-70) for sharded renders.
 * Multi-process (torch.distributed) callers gather mcpt_accum_device_ptr with RCCL instead.
 * Asynchronous; mcpt_read_accum(frame) synchronizes. */
int mcpt_gather_rows(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards);
/* mcpt_gather_rows for shards with per-pixel sample counts (adaptive sampling): the
 * same peer copies, stream ordering in both directions and device / event restore, but the shards
 * may hold different pass counts and each shard's counts travel with its rows into `frame`'s count
 * plane (one int32 per pixel, 4 B/px, allocated by the first counted gather after a
 * mcpt_set_target* and freed by the next mcpt_set_target* / mcpt_destroy).  A shard with the
 * adaptive mode on contributes its pixels' counts (mcpt_read_sample_counts' values), a shard with
 * the mode off its pass count for all its pixels; frame's pass count becomes the largest shard pass
 * count.  Every row of `frame` (a full-frame target in row order) must be held by exactly one
 * shard, else MCPT_ERR_INVALID_ARG: no pixel is left with count 0.  Afterwards `frame` has
 * per-pixel counts: mcpt_read_sample_counts and mcpt_read_resolved serve the plane and
 * mcpt_denoise_resolved filters the frame (mcpt_denoise_resolved_guided returns MCPT_ERR_NO_STATS
 * until the shards' error maps have been gathered too: mcpt_gather_error_map below).  The plane stays valid until frame's accumulator changes:
 * mcpt_set_target*, mcpt_clear_accum, mcpt_write_accum, mcpt_checkpoint_load, mcpt_gather_rows and
 * any mcpt_render* into `frame` invalidate it.  The multi-process (torch.distributed / RCCL) gather
 * carries counts through mcpt_pack_counted_device and mcpt_load_rows_counted below. */
int mcpt_gather_rows_counted(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards);

/* The counted gather across processes (mcpt/dist.py ShardedRenderer.gather_counted):
 * each rank packs its shard, the caller's collective moves the packed rows to one rank, and that rank
 * loads them into a full-frame context.  A packed record is 16 bytes per pixel, {r, g, b, count}: the
 * accumulator's three f32 words bit for bit and the pixel's int32 sample count; rows in local order,
 * n_local x W records.  Nothing on the way may read the words as floats (sums may be inf or NaN,
 * counts are denormal bit patterns): carry them as int32.
 *
 * mcpt_pass_count: the accumulator's pass count (what mcpt_read_accum reports) without the copy;
 * host only, no synchronization.
 * mcpt_pack_counted_device: the local accumulator and every pixel's sample count into `dst_dev`
 * (16-byte aligned, `bytes` >= n_local x W x 16, else MCPT_ERR_INVALID_ARG; MCPT_ERR_NO_TARGET without a
 * target).  The count is chosen as mcpt_gather_rows_counted chooses a shard's: the count plane when
 * valid, else the adaptive mode's per-pixel counts, else the pass count for every pixel; any target,
 * mode on or off.  One kernel on the context's stream, ordered after the queued renders like
 * mcpt_copy_accum_device; asynchronous.
 * mcpt_load_rows_counted: `frame` (a full-frame target in row order) <- packed rows on frame's
 * device: frame row y from row src_row[y] of the src_rows x W records at `src_dev` (16-byte aligned).
 * src_row: H ints on the host, each in [0, src_rows); pass_count > 0; else MCPT_ERR_INVALID_ARG and
 * `frame` keeps what it has.  One kernel on frame's stream writes the sums to the accumulator and the
 * counts to the count plane (allocated and freed as mcpt_gather_rows_counted's); asynchronous.  The
 * index is uploaded when it differs from the previous call's (replacing one waits for the stream).
 * Afterwards `frame` is in the state mcpt_gather_rows_counted leaves: per-pixel counts from the plane,
 * its pass count = pass_count, mcpt_read_sample_counts / mcpt_read_resolved / mcpt_denoise_resolved
 * serve it, mcpt_denoise_resolved_guided returns MCPT_ERR_NO_STATS (until mcpt_load_rows_error_map
 * below), and the same calls invalidate the plane. */
int mcpt_pass_count(mcpt_ctx* ctx, int* pass_count);
int mcpt_pack_counted_device(mcpt_ctx* ctx, void* dst_dev, size_t bytes);
int mcpt_load_rows_counted(mcpt_ctx* frame, const void* src_dev, long long src_rows, const int* src_row,
                           int pass_count);

/* The GATHERED ERROR MAP of a frame context: the shards' error maps {se, r},
 * which are per pixel and do not depend on the partition, moved to the context that holds the
 * gathered frame, so that the noise-guided filters serve sharded renders.  State: a device plane of
 * H x W x {se, r} f32 (8 B per pixel) with a validity flag, allocated by the first call that fills it
 * after a mcpt_set_target* and freed by the next mcpt_set_target* / mcpt_destroy, alongside the count
 * plane.  It describes the accumulator the frame holds, so everything that invalidates the count
 * plane invalidates it: mcpt_set_target*, mcpt_clear_accum, mcpt_write_accum, mcpt_checkpoint_load,
 * mcpt_gather_rows, mcpt_gather_rows_counted, mcpt_load_rows_counted and any mcpt_render* into the
 * frame.  The order of use is therefore: gather the rows (plain or counted), then gather the map.
 * The row gathers themselves are unchanged and carry no map.
 *
 * While the plane is valid, mcpt_denoise_guided (a plainly gathered frame of uniform shards) and
 * mcpt_denoise_resolved_guided (a frame with a count plane) read it in place of the context's own
 * window map, mcpt_read_error_map returns it (H x W x 2 f32), and mcpt_error_map_record reduces it.
 * Without one all of them behave as before (MCPT_ERR_NO_STATS on a gathered frame).
 *
 * mcpt_gather_error_map: inside one process; peer copies of every shard's map rows into the plane at
 * their global rows, one hipMemcpyPeerAsync per run of consecutive global rows, with
 * mcpt_gather_rows_counted's stream ordering in both directions and device / event restore.
 * `frame`: a full-frame target in row order with the shards' W x H; every frame row held by exactly
 * one shard (else MCPT_ERR_INVALID_ARG); every shard with statistics on and an error map of its
 * current window (else MCPT_ERR_NO_STATS), written by mcpt_convergence (uniform shards) or
 * mcpt_adaptive_select (adaptive shards: retired blocks contribute their stored entries).  On any
 * error the plane is left invalid.  Asynchronous.
 * mcpt_pack_error_map_device: across processes, the sending end; the shard's n_local x W map entries
 * in local row order into `dst_dev` (8-byte aligned, `bytes` >= n_local x W x 8, else
 * MCPT_ERR_INVALID_ARG; MCPT_ERR_NO_TARGET without a target, MCPT_ERR_NO_STATS without a current map),
 * a device-to-device copy on the context's stream after the queued work.  The words travel as bits
 * (se may be inf or NaN for an overflowed pixel): carry them as int32, like the packed rows.
 * mcpt_load_rows_error_map: the receiving end; frame row y of the plane from row src_row[y] of the
 * src_rows x W 8-byte records at `src_dev` (8-byte aligned), one kernel on frame's stream that moves
 * the records as integers; asynchronous.  The index contract is mcpt_load_rows_counted's (H host ints
 * in [0, src_rows), else MCPT_ERR_INVALID_ARG), and the device copy of the index is shared with it: a
 * counted load and a map load with the same index upload it once.  On any error the plane is left
 * invalid.
 * mcpt_error_map_record: the frame-level record of whichever map is current on the context: the
 * gathered plane when valid, else the context's own window map, else MCPT_ERR_NO_STATS.  n_px,
 * n_above = #{r > threshold}, max_r, sum_q and mean_r as mcpt_convergence defines them, reduced from
 * the STORED r values (neither se nor r is recomputed), so the records of the shards' last
 * mcpt_convergence / mcpt_adaptive_select with the same threshold add up to it; passes = the
 * context's pass count for a gathered plane (batches = 0), the window's passes and batches for an own
 * map.  Positive finite threshold, else MCPT_ERR_INVALID_ARG.  Synchronizes.
 * mcpt_error_map_source: 0 no map, 1 the context's own window map, 2 the gathered plane; host only. */
struct mcpt_convergence_t;   /* (defined with mcpt_convergence below) */
int mcpt_gather_error_map(mcpt_ctx* frame, mcpt_ctx* const* shards, int n_shards);
int mcpt_pack_error_map_device(mcpt_ctx* ctx, void* dst_dev, size_t bytes);
int mcpt_load_rows_error_map(mcpt_ctx* frame, const void* src_dev, long long src_rows, const int* src_row);
int mcpt_error_map_record(mcpt_ctx* ctx, float threshold, struct mcpt_convergence_t* out);
int mcpt_error_map_source(mcpt_ctx* ctx, int* source);

/* Select the traversal strategy (mcpt_traversal) for later renders; default AUTO.  AUTO times
 * its schedule candidates on the first launches of >= 2^24 samples after a scene upload — the
 * per-lane walk; the wave-coherent walk (BVH depth < 8 only); the per-lane walk with two and
 * with four pass segments per work item (where the launch has that many segments); for BVH
 * depth >= 8 also the per-lane walk with the deep knobs (leaf batch 16, walk exit 40, min-done 8)
 * at four and at eight segments per item — at most five candidates, each timed twice (forward,
 * then reverse order; each one's best time per sample kept), compared only between launches of
 * the same shape: at most 10 trial launches, run in order on the context's stream (not on the
 * render lanes); a trial's time is read when the call after the next one starts, so AUTO settles
 * two calls after its last trial (mcpt.AUTO_TRIALS = 12 calls).  It never times the stream
 * schedule, which runs only when selected explicitly (MCPT_TRAVERSAL_STREAM).  Later launches of
 * that shape use the fastest — except that, with render lanes on, two segments per item give way
 * to four when the four-segment trials are within 2 % (on the lanes, longer items overlap the
 * previous launch's tail better than the in-order trials show).  mcpt_get_walk_exit /
 * mcpt_get_leaf_batch report the knobs of the
 * candidate the next launch uses.
 * mcpt_get_traversal reports the strategy the next render uses (a trial candidate until AUTO
 * has settled: see mcpt_get_schedule's `settled`).  Every strategy gives the same bits. */
int mcpt_set_traversal(mcpt_ctx* ctx, int mode);
int mcpt_get_traversal(mcpt_ctx* ctx, int* resolved_mode);
/* The whole schedule the next launch of the last launch shape uses: traversal mode, pass
 * segments per work item (MCPT_SEG_PER_ITEM env overrides), and whether AUTO has finished its
 * timing trials (1; always 1 for a fixed mode).  Any pointer may be NULL.  No reference
 * equivalent (the fragment shader has one fixed schedule). */
int mcpt_get_schedule(mcpt_ctx* ctx, int* traversal, int* seg_per_item, int* settled);

/* Per-lane walks (MCPT_TRAVERSAL_LANE): the wave suspends its BVH walk loop once at most
 * `lanes` lanes are still walking, shades the finished lanes and resumes the rest with
 * their next rays (0 = never suspend; -1 = default: 24 with mesh instances, 16 for BVH
 * depth >= 8, else 0).  Same
 * results for every value; a scheduling knob.  mcpt_get_walk_exit reports the value used. */
int mcpt_set_walk_exit(mcpt_ctx* ctx, int lanes);
int mcpt_get_walk_exit(mcpt_ctx* ctx, int* resolved_lanes);

/* Stream schedule (MCPT_TRAVERSAL_STREAM) knobs: path slots (0 = default 16 Mi; never more than
 * the launch's (pixel, pass segment) units; 248 B of device memory per slot, in two pools: 4 GB
 * per context at the default, allocated at the first stream render and freed when
 * mcpt_set_traversal selects another schedule)
 * and the trace kernel's refill threshold (a wave takes new rays for its idle lanes once at
 * most `refill` lanes still walk; 0 = only when all are done; -1 = default 56).  Same results
 * for every value.  mcpt_stream_iterations: trace + shade iterations of the last stream launch
 * (0 if it did not use the stream schedule).  No reference equivalent. */
int mcpt_set_stream_pool(mcpt_ctx* ctx, int slots, int refill);
int mcpt_stream_iterations(mcpt_ctx* ctx, long long* iterations);

/* Per-lane walks: run the primitive-test block only once at least `lanes` lanes wait on a
 * leaf (or no lane can take a node step); others wait (0 = off: node and leaf blocks every
 * iteration; -1 = default: 8 for BVH depth >= 8, else 0).  Same results for every value. */
int mcpt_set_leaf_batch(mcpt_ctx* ctx, int lanes);
int mcpt_get_leaf_batch(mcpt_ctx* ctx, int* resolved_lanes);

/* Render lanes (round 6): once the schedule is settled, the sub-launches of render calls
 * alternate between two internal lanes (HIP streams with their own segment-sum buffers and
 * work-item order state), so a launch's render kernel starts while the previous launch's last
 * workgroups still run; the combines stay in call order on the context's stream, which is
 * ordered after all lane work (results are the same bits).  on = 0: every launch in order on the
 * context's stream.  Default 1 (environment MCPT_OVERLAP=0: 0). */
int mcpt_set_render_lanes(mcpt_ctx* ctx, int on);

/* Bound (bytes) of the device buffer holding the per-chunk partial sums of one launch.  A
 * render call whose pass range spans more 32-pass chunks than fit is run as several launches
 * cut at chunk boundaries (e.g. 84,000 passes at 4K in one call); the accumulator is
 * bit-identical for any budget.  Default 4 GiB (env MCPT_PARTIAL_BYTES at create). */
int mcpt_set_partial_budget(mcpt_ctx* ctx, size_t bytes);
/* (Device memory of a context: the accumulator (12 B per local pixel), the segment sums (up to
 * this budget, allocated by the first launch that needs them) and, with the stream schedule,
 * its pools; the scene buffers.) */
/* Sub-launches the last render call was split into. */
int mcpt_last_launch_count(mcpt_ctx* ctx, int* n_launches);
/* 1 if the last render call ran one pass segment per pass: a call of 2..256 passes whose
 * launch would have fewer than 4 work items per compute unit (e.g. 256x256 at 4 spp) runs each
 * pass as its own segment, so a pixel's passes run side by side, and the combine step sums each
 * 32-pass chunk's passes from 0 in pass order, as one lane would: the bits do not change.
 * Env MCPT_PASS_SPLIT=0/1 forces it off/on. */
int mcpt_last_pass_split(mcpt_ctx* ctx, int* split);

/* Ray queries on the uploaded scene — the shader library calls a TP integrator may use
 * (raytracer_func.frag:718-781, 874-907): traverse_all_bvh (any_hit = 0) or just_hit_bvh
 * (any_hit = 1: stop at the first primitive hit), or with prim >= 0 intersect_one_prim /
 * hit_one_prim (that primitive only), then intersection_info / _color_info / _mat_info.
 * origins, dirs: n × 3 f32 host arrays (directions used as given, like the shader).  A miss
 * has shape = -1, dist = FLT_MAX and zero N/P/colour/material.  Synchronous. */
typedef struct mcpt_hit {
  int shape;          /* primitive type code of the hit (0 mesh, 1 sphere .. 5 quad), -1 = miss */
  int prim;           /* primitive index (after sortEmissiveFirst) */
  int dir;            /* face / part code of the hit (closest_intersection.dir); for a mesh
                         hit the mesh-local triangle index (Mesh_intersect's tri_index) */
  float dist;         /* world distance from the origin */
  float pl[3], pg[3]; /* hit point in primitive space / world space */
  float N[3], P[3];   /* intersection_info: normal and position */
  float color[4];     /* intersection_color_info (rgb, opacity) */
  float material[4];  /* intersection_mat_info (shininess, roughness, emissivity, area) */
} mcpt_hit;
int mcpt_trace(mcpt_ctx* ctx, const float* origins, const float* dirs, int n, int any_hit, int prim,
               mcpt_hit* out);

/* Guide buffers (AOVs) and the edge-avoiding a-trous denoiser (no reference
 * equivalent: fs_frag only averages).  Device memory: 80 B per local pixel (guides 32, albedo 16,
 * two filter buffers 16 each), allocated by the first of these calls after a mcpt_set_target* and
 * freed by the next mcpt_set_target* / mcpt_destroy.  No render call does any work for them.
 *
 * mcpt_render_guides: per local pixel the primary hit of its camera ray (the render kernel's ray:
 * invPV, invV as mcpt_render takes them) — normal, world position, distance, primitive key, and
 * the hit primitive's colour.  Works on any target, row shards included.  Asynchronous on the
 * context's stream.  mcpt_set_target*, mcpt_upload_scene, mcpt_upload_meshes and
 * mcpt_set_flat_face invalidate the guides (MCPT_ERR_NO_GUIDES until rendered again).
 * mcpt_read_guides: guide8 = n_local x 8 f32 {N.xyz, key as int32 bits, P.xyz, dist} with key =
 * shape << 28 | primitive index (a miss: key -1, N = P = 0, dist = FLT_MAX); albedo4 = n_local x 4
 * f32 rgba (0 on a miss).  Either pointer may be NULL.  Synchronizes. */
int mcpt_render_guides(mcpt_ctx* ctx, const float* invPV, const float* invV);
int mcpt_read_guides(mcpt_ctx* ctx, float* guide8, float* albedo4);
/* `iterations` (0..8) a-trous passes (tap spacing 1, 2, 4, ...) over accum / pass_count, guided by
 * the guide buffers; the weights' arithmetic is fixed bit for bit, 0 iterations
 * give accum / pass_count itself.  The accumulator and the pass count are not touched, so a
 * progressive render goes on afterwards.  Needs a full-frame target in row order (local row i =
 * global row i; after mcpt_gather_rows for sharded renders) and pass_count > 0, positive finite
 * sigmas (else MCPT_ERR_INVALID_ARG), and current guides (else MCPT_ERR_NO_GUIDES).  Asynchronous,
 * ordered after the queued renders.  sigma_color: colour distance (in radiance units) at which a
 * tap's weight falls to 1/4 in the first iteration (halved each iteration); sigma_plane: the same
 * for a tap's distance from the centre's tangent plane, in world units per pixel of tap spacing.
 * Env MCPT_DENOISE_NAIVE=1: every tap from global memory; =0: steps 1 and 2 from LDS tiles (the A/B
 * of DESIGN.md §3.7; same bits). */
int mcpt_denoise(mcpt_ctx* ctx, int iterations, float sigma_color, float sigma_plane);
/* the last mcpt_denoise's image, n_local x 3 f32.  Synchronizes. */
int mcpt_read_denoised(mcpt_ctx* ctx, float* rgb_out);
/* Device times (HIP events) of the last mcpt_render_guides and the last mcpt_denoise (its average
 * and iterations); 0 for what has not run.  Either pointer may be NULL.  Waits for them.
 * mcpt_denoise_iteration_ms: iteration 0 .. iterations-1 of the last mcpt_denoise alone (-1: its
 * averaging step). */
int mcpt_last_denoise_ms(mcpt_ctx* ctx, float* guides_ms, float* filter_ms);
int mcpt_denoise_iteration_ms(mcpt_ctx* ctx, int iteration, float* ms);
/* Which kernel the last mcpt_denoise's iterations ran: bit s of *lds_mask set = iteration s
 * staged its taps in LDS, clear = it read them from global memory (the same bits either way). */
int mcpt_last_denoise_path(mcpt_ctx* ctx, int* lds_mask);

/* Noise statistics, the convergence metric and the noise-guided filter (no
 * reference equivalent).  Opt-in: with statistics off no render call does any work for them.
 * Device memory while on: +16 B per local pixel for the state, +8 B per local pixel for the error
 * map, allocated by the first mcpt_stats_begin after a mcpt_set_target* and freed by mcpt_stats_end,
 * the next mcpt_set_target* (which turns statistics off) and mcpt_destroy.  Works on any target, row
 * shards included: the records of shards add (n_px, n_above, sum_q) and max (max_r).
 *
 * The statistics are batch means of the pixels' luminance sums over a window of render calls:
 * mcpt_stats_begin snapshots the accumulator and starts a window (passes = batches = 0;
 * asynchronous); from then on every mcpt_render / mcpt_render_counted of n_passes > 0 appends one
 * batch of its n_passes, enqueued on the context's stream behind the call's last combine without a
 * host wait, whatever the schedule and however many launches the call runs.  mcpt_clear_accum,
 * mcpt_write_accum, mcpt_checkpoint_load and mcpt_gather_rows* do not touch the statistics: after
 * them the caller declares the accumulator's n new passes as a batch (mcpt_stats_add_batch, n > 0;
 * asynchronous) or begins again.  mcpt_checkpoint_save's files do not store statistics: a render
 * resumed from one begins a new window (mcpt_adaptive_checkpoint_save's do).
 *
 * mcpt_convergence: per local pixel the standard error `se` of the window's mean luminance and the
 * relative error r = se / (max(0, mean) + mu_floor), clamped to 64 (an overflowed pixel counts 64),
 * written to the error map, and the frame's record: n_px, n_above = #{r > threshold}, max_r, and
 * sum_q = the sum of trunc(r * 65536) (an integer: the same bits for any reduction order);
 * mean_r = sum_q / 65536 / n_px.  Needs statistics on and two batches or more (else
 * MCPT_ERR_NO_STATS), positive finite threshold and mu_floor (else MCPT_ERR_INVALID_ARG).
 * Synchronizes.  mcpt_read_error_map: n_local x 2 f32 {se, r} of the window's last
 * mcpt_convergence (MCPT_ERR_NO_STATS without one); on a context with a valid gathered error map
 * (mcpt_gather_error_map), H x W x 2 f32 of that map.  Synchronizes.
 *
 * mcpt_denoise_guided: mcpt_denoise with the colour term's width taken per pixel from the error
 * map, k_color * se (halved each iteration), in place of sigma_color; mcpt_denoise's preconditions
 * plus an error map (else MCPT_ERR_NO_STATS): the gathered error map when the context holds a valid
 * one (sharded renders: mcpt_gather_error_map), else the current window's, read as the last
 * mcpt_convergence wrote it.  It writes mcpt_denoise's result buffers: mcpt_read_denoised,
 * mcpt_last_denoise_ms, mcpt_denoise_iteration_ms and mcpt_last_denoise_path serve both filters.
 *
 * mcpt_last_stats_ms: device times (HIP events) of the last batch update and the last error kernel;
 * 0 for what has not run.  Either pointer may be NULL.  Waits for them. */
int mcpt_stats_begin(mcpt_ctx* ctx);
int mcpt_stats_end(mcpt_ctx* ctx);
int mcpt_stats_add_batch(mcpt_ctx* ctx, int n);
/* on / passes / batches of the window (0 / 0 / 0 with statistics off); any pointer may be NULL */
int mcpt_stats_info(mcpt_ctx* ctx, int* on, long long* passes, int* batches);
typedef struct mcpt_convergence_t {
  long long n_px, n_above;
  unsigned long long sum_q;
  float max_r;
  double mean_r;
  long long passes;
  int batches;
} mcpt_convergence_t;
int mcpt_convergence(mcpt_ctx* ctx, float threshold, float mu_floor, mcpt_convergence_t* out);
int mcpt_read_error_map(mcpt_ctx* ctx, float* se_r2);
int mcpt_denoise_guided(mcpt_ctx* ctx, int iterations, float k_color, float sigma_plane);
int mcpt_last_stats_ms(mcpt_ctx* ctx, float* update_ms, float* error_ms);

/* The variance-propagating filter ("Variance filter"; no reference equivalent).
 * The error map's se^2 is prefiltered over each pixel's 3x3 neighbours of its own key, rides in the
 * filter image's fourth word and is filtered with the squared weights; iteration s takes its
 * colour tolerance from the variance its input has: kc_p = 1 / (k_color^2 * var_p + 2^-40), not
 * halved.  Plane and normal terms, taps and kernels are mcpt_denoise's.
 *
 * mcpt_denoise_variance: preconditions, error codes and error-map source exactly those of
 * mcpt_denoise_guided (the gathered plane when valid, else the own window's map, else
 * MCPT_ERR_NO_STATS; MCPT_ERR_INVALID_ARG once an adaptive block has retired).
 * mcpt_denoise_resolved_variance: those of mcpt_denoise_resolved_guided (MCPT_ERR_NO_ADAPTIVE
 * without per-pixel counts); with no block retired it gives mcpt_denoise_variance's bits.
 * Both write mcpt_denoise's result buffers and allocate nothing beyond them: mcpt_read_denoised,
 * mcpt_last_denoise_ms, mcpt_denoise_iteration_ms (-1: the averaging / resolve step, which holds
 * the prefilter) and mcpt_last_denoise_path serve them.
 * mcpt_read_denoised_variance: n_local f32, the fourth word of the last variance filter's image
 * (iterations = 0: the prefiltered variance); MCPT_ERR_NO_STATS if the last filter run was not a
 * variance filter.  Synchronizes. */
int mcpt_denoise_variance(mcpt_ctx* ctx, int iterations, float k_color, float sigma_plane);
int mcpt_denoise_resolved_variance(mcpt_ctx* ctx, int iterations, float k_color, float sigma_plane);
int mcpt_read_denoised_variance(mcpt_ctx* ctx, float* v_out);

/* Adaptive sampling of 8x8 pixel blocks guided by the error map (no reference
 * equivalent).  Opt-in, on top of the noise statistics; with the mode off nothing changes.
 *
 * A block is 8 local rows x 8 columns of the local grid (a wave of the render kernel):
 * blocks_x = ceil(W / 8), blocks_y = ceil(local rows / 8), id = by * blocks_x + bx; any target, row
 * shards included.  While the mode is on a block holds an active flag and the passes rendered into
 * it since mcpt_adaptive_begin; a pixel's sample count is the accumulator's pass count at
 * mcpt_adaptive_begin plus its block's passes.  Blocks only ever leave the active set, so an active
 * block has received every pass so far and every pixel holds, bit for bit, what a uniform render
 * of the same calls held after that pixel's sample count.  Device memory: 12 B per
 * block, allocated by mcpt_adaptive_begin, freed by mcpt_adaptive_end, mcpt_stats_end, the next
 * mcpt_set_target* (all of which turn the mode off) and mcpt_destroy.
 *
 * mcpt_adaptive_begin: needs statistics on (else MCPT_ERR_NO_STATS); every block active, zero
 * passes; a block is not retired before it holds min_passes (>= 0) passes.  Asynchronous.
 * mcpt_adaptive_select: for every active block the {se, r} of its pixels as mcpt_convergence
 * computes them, written to the error map; the block stays active iff its largest r > threshold or
 * it holds fewer than min_passes passes.  Retired blocks are not computed, keep their map entries
 * and never return.  The record is mcpt_convergence's over all local pixels (fresh values of active
 * blocks, stored ones of retired blocks) plus n_active_blocks, n_blocks and samples = the sum of
 * all pixels' sample counts.  Arguments and preconditions as mcpt_convergence; synchronizes.
 * mcpt_read_error_map reads the map.  mcpt_convergence itself is unchanged and knows nothing of
 * retired blocks (their window sums stop growing while the window's pass count does not): with the
 * adaptive mode on, use mcpt_adaptive_select.
 * mcpt_read_active_blocks: the active block ids of the last select (all blocks before the first),
 * ascending; *n = how many, at most `capacity` of them copied.
 * mcpt_render_adaptive: mcpt_render for the active blocks only, on the context's stream; their pass
 * counts and the context's pass count grow by n_passes, and the call is one statistics batch.  An
 * empty list launches nothing, changes nothing and returns MCPT_OK.  The schedule (AUTO's trials,
 * work-item order, render lanes, mcpt_last_render_ms) takes no part and is left as it was.
 * A plain mcpt_render while the mode is on is allowed: it renders every pixel and adds n_passes to
 * every block's count, retired ones too.
 * mcpt_read_sample_counts: n_local ints, a pixel's sample count.  mcpt_read_resolved: n_local x 3
 * f32, accum / (float)count per channel (mcpt_average's division with the pixel's own count).
 * mcpt_adaptive_info: any pointer may be NULL (0 / 0 / 0 with the mode off).
 * mcpt_last_adaptive_ms: device times (HIP events) of the last select (with its list scan) and the
 * last adaptive render (with its combines); 0 for what has not run.  Waits for them.
 * With the mode off the other calls return MCPT_ERR_NO_ADAPTIVE.
 *
 * mcpt_denoise, mcpt_denoise_guided, mcpt_checkpoint_save, mcpt_gather_rows, mcpt_read_accum's pass
 * count and mcpt_clear_accum / mcpt_write_accum know nothing of per-pixel counts (end the mode
 * before replacing the accumulator).  Once a block has retired, mcpt_denoise and mcpt_denoise_guided
 * return MCPT_ERR_INVALID_ARG instead of an image divided by the wrong count; the forms below
 * filter, checkpoint and gather frames with per-pixel counts.
 *
 * A context HAS PER-PIXEL SAMPLE COUNTS when (a) the adaptive mode is on (the count of a pixel is
 * the pass count at mcpt_adaptive_begin plus its block's passes) or (b) a counted gather has filled
 * its count plane: mcpt_gather_rows_counted inside one process, or mcpt_load_rows_counted from the
 * packed rows a multi-process gather delivered.  The resolved colour of a pixel is accum /
 * (float)count per channel, mcpt_read_resolved's bits; mcpt_read_sample_counts and
 * mcpt_read_resolved serve both cases (MCPT_ERR_NO_ADAPTIVE with neither).
 *
 * mcpt_denoise_resolved / mcpt_denoise_resolved_guided: mcpt_denoise / mcpt_denoise_guided with the
 * resolved colour as the input image in place of accum / pass_count; the same preconditions
 * (full-frame target in row order, current guides, 0..8 iterations, positive finite sigmas), the
 * same filter kernels and the same result buffers (mcpt_read_denoised, mcpt_last_denoise_ms,
 * mcpt_denoise_iteration_ms with -1 the resolve step, mcpt_last_denoise_path).  A context without
 * per-pixel counts returns MCPT_ERR_NO_ADAPTIVE.  The guided form needs the error map of the
 * current window (the last mcpt_adaptive_select's), else MCPT_ERR_NO_STATS; on a gathered frame
 * (case b) it needs a GATHERED ERROR MAP (below) and returns MCPT_ERR_NO_STATS without one, whatever
 * window the frame context runs itself.  With no block retired the resolved forms give
 * mcpt_denoise's bits.
 *
 * Both gathers carry the counts: in one process mcpt_gather_rows_counted, across processes
 * (torch.distributed / RCCL, mcpt/dist.py) mcpt_pack_counted_device on every rank and
 * mcpt_load_rows_counted on the receiving one.  The shards' error maps do not travel with them:
 * they travel through the separate calls declared after the counted gather's (the gathered error
 * map), after which the guided filters serve the gathered frame. */
typedef struct mcpt_adaptive_t {
  long long n_px, n_above;
  unsigned long long sum_q;
  float max_r;
  double mean_r;
  long long passes;
  int batches;
  long long n_active_blocks, n_blocks;
  long long samples;
} mcpt_adaptive_t;
int mcpt_adaptive_begin(mcpt_ctx* ctx, int min_passes);
int mcpt_adaptive_end(mcpt_ctx* ctx);
int mcpt_adaptive_select(mcpt_ctx* ctx, float threshold, float mu_floor, mcpt_adaptive_t* out);
int mcpt_read_active_blocks(mcpt_ctx* ctx, int* ids, int capacity, int* n);
int mcpt_render_adaptive(mcpt_ctx* ctx, const float* invPV, const float* invV, int first_pass, int n_passes,
                         float date, int bounces, float refract_ind, int variant);
int mcpt_read_sample_counts(mcpt_ctx* ctx, int* counts);
int mcpt_read_resolved(mcpt_ctx* ctx, float* rgb);
int mcpt_adaptive_info(mcpt_ctx* ctx, int* on, long long* n_active, long long* n_blocks);
int mcpt_last_adaptive_ms(mcpt_ctx* ctx, float* select_ms, float* render_ms);
int mcpt_denoise_resolved(mcpt_ctx* ctx, int iterations, float sigma_color, float sigma_plane);
int mcpt_denoise_resolved_guided(mcpt_ctx* ctx, int iterations, float k_color, float sigma_plane);

/* Adaptive sampling that stops on the DENOISED frame's error (no reference
 * equivalent): mcpt_adaptive_select's twin whose rule reads the variance the variance-propagating
 * filter leaves in its image, so that a block retires once the image mcpt_denoise_resolved_variance
 * shows of it meets the threshold.  One call, three steps on the context's stream:
 *   A  for every active block the {se, r} of its pixels into the error map and the raw record, as
 *      mcpt_adaptive_select computes them; no block retires.  Retired blocks keep their entries.
 *   B  exactly what mcpt_denoise_resolved_variance(ctx, iterations, k_color, sigma_plane) would run
 *      now: the resolve and the 3x3 prefilter of the map step A wrote, then the iterations, into the
 *      same result buffers with the same bits.
 *   C  for every local pixel, with c = {r, g, b, v} step B's result, in binary32 without
 *      contraction in the order written:
 *        Yf = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b;  sef = sqrt(c.v);
 *        rf = sef / (max(0, Yf) + mu_floor);  rf = 64 if Yf is not finite or not rf <= 64.
 *      An active block stays active iff its largest rf > threshold, or its largest r (step A's map
 *      entries) > raw_cap, or it holds fewer than min_passes passes; the maxima run over the
 *      block's in-frame pixels.  Retired blocks never return.  The active list is rebuilt as
 *      mcpt_adaptive_select rebuilds it.
 * raw_cap keeps a block whose filtered variance is small only because a wide colour tolerance
 * blurred it while its raw error is still large; r is clamped to 64, so raw_cap = 64 turns the guard
 * off, and raw_cap = threshold keeps every block mcpt_adaptive_select would keep.
 *
 * The record: `raw` is mcpt_adaptive_select's record of the same state (n_px, n_above, sum_q, max_r,
 * mean_r, passes, batches, samples, n_blocks as that call defines them) with n_active_blocks = the
 * blocks THIS rule keeps; n_above_f, sum_qf (sum of trunc(rf * 65536)), max_rf and mean_rf =
 * sum_qf / 65536 / n_px are the same record of rf over ALL local pixels, retired blocks' included
 * (their rf comes from the filter like everyone's).  Integer sums and a maximum: the bits do not
 * depend on the order.
 *
 * Preconditions, in this order: adaptive mode on (else MCPT_ERR_NO_ADAPTIVE); threshold, raw_cap,
 * mu_floor, k_color and sigma_plane positive and finite, iterations in 0..8, a full-frame target in
 * row order that holds passes and no gathered count plane or gathered error map (else
 * MCPT_ERR_INVALID_ARG); statistics on with two batches or more (else MCPT_ERR_NO_STATS); current
 * guides (else MCPT_ERR_NO_GUIDES).  On any of these nothing changes: not the flags, the map or the
 * result buffers.
 *
 * Afterwards the error map is valid as after a select (mcpt_read_error_map), and the filter's result
 * buffers hold step B's image as a variance filter's: mcpt_read_denoised, mcpt_read_denoised_variance,
 * mcpt_last_denoise_ms, mcpt_denoise_iteration_ms and mcpt_last_denoise_path serve it, so every check
 * leaves the current denoised preview.  mcpt_last_adaptive_ms's select time is steps A + C with the
 * list scan (step B's is mcpt_last_denoise_ms's filter time).  mcpt_adaptive_select and this call may
 * alternate freely: both only retire.  Checkpoints need nothing new: the rule is a function of the
 * accumulator, the counts, the statistics state, the stored map and the guides, and the guides are
 * rendered again after mcpt_adaptive_checkpoint_load.  Device memory: one more block of partial
 * records beside the statistics' (4 KiB), nothing per pixel.  Synchronizes once, at the end, for the
 * record. */
typedef struct mcpt_adaptive_filtered_t {
  mcpt_adaptive_t raw;
  long long n_above_f;
  unsigned long long sum_qf;
  float max_rf;
  double mean_rf;
} mcpt_adaptive_filtered_t;
extern int mcpt_adaptive_select_filtered(mcpt_ctx* ctx, float threshold, float raw_cap, float mu_floor, int iterations,
                                         float k_color, float sigma_plane, mcpt_adaptive_filtered_t* out);

/* Queued adaptive runs (no reference equivalent): `rounds` rounds of an adaptive
 * render loop on the context's stream with ONE host wait, at the end.  The call is equivalent, bit
 * for bit in every piece of state and every record, to this loop over the calls above:
 *   for i in 0 .. rounds-1:
 *     if the active list is empty: stop
 *     mcpt_render_adaptive(first_pass + i * n_passes, n_passes, ...)
 *     if the window holds >= 2 batches and ((i + 1) % check_every == 0 or i == rounds - 1):
 *       mcpt_adaptive_select(threshold, mu_floor, &records[k++])
 * (mcpt_adaptive_run_filtered: mcpt_adaptive_select_filtered with its further arguments).  State is
 * the accumulator, the block flags and passes, the active list and its length, the statistics state
 * and the error map, the pass count, the window's passes and batches and, for the filtered form, the
 * filter's result buffers: afterwards every other call continues as if the loop had run.  The host
 * sizes the launches from the list's length on entry (lists only shrink); the kernels read the length
 * each round has from the device, and the rounds queued behind the select that emptied the list leave
 * every buffer as it is.  records[k] are the loop's, in order; out: rounds_queued = rounds,
 * rounds_run / selects_run / passes_run what the loop would have rendered and selected, device_ms
 * the whole run between two HIP events.  mcpt_last_adaptive_ms / mcpt_last_stats_ms /
 * mcpt_last_denoise_ms report the last QUEUED round and select of the run.
 * Preconditions, checked before anything is enqueued (a refusal changes nothing): those of
 * mcpt_render_adaptive, then those of the matching select except its two batches (the schedule's),
 * in those calls' order; then MCPT_ERR_INVALID_ARG for n_passes <= 0, rounds outside
 * 1..MCPT_ADAPTIVE_RUN_MAX_ROUNDS, check_every <= 0, records_capacity below the selects the
 * schedule can run, or records NULL with records_capacity > 0.  A list that is empty on entry
 * enqueues nothing: MCPT_OK with rounds_run = 0.  Device memory: 1 MiB of partial records per rule
 * (MCPT_ADAPTIVE_RUN_MAX_ROUNDS x 4 KiB) with the statistics buffers' lifetime. */
#define MCPT_ADAPTIVE_RUN_MAX_ROUNDS 256
typedef struct mcpt_adaptive_run_t {
  int rounds_queued;      /* = rounds */
  int rounds_run;         /* rounds the equivalent host loop would have rendered */
  int selects_run;        /* records[] entries filled */
  long long passes_run;   /* rounds_run * n_passes */
  float device_ms;        /* HIP events around the whole run */
} mcpt_adaptive_run_t;
extern int mcpt_adaptive_run(mcpt_ctx* ctx, const float* invPV, const float* invV, int first_pass, int n_passes, int rounds,
                             int check_every, float threshold, float mu_floor, float date, int bounces,
                             float refract_ind, int variant, mcpt_adaptive_t* records, int records_capacity,
                             mcpt_adaptive_run_t* out);
extern int mcpt_adaptive_run_filtered(mcpt_ctx* ctx, const float* invPV, const float* invV, int first_pass, int n_passes,
                               int rounds, int check_every, float threshold, float raw_cap, float mu_floor,
                               int iterations, float k_color, float sigma_plane, float date, int bounces,
                               float refract_ind, int variant, mcpt_adaptive_filtered_t* records, int records_capacity,
                               mcpt_adaptive_run_t* out);

/* The host side of that schedule: the next step of a loop that renders batches of `batch` passes for
 * the active blocks, selects after every check_every calls (from the second on, and at the cap) and
 * ends at max_passes, after `done` passes in `calls` render calls (a queued run of r rounds counts as
 * r; a resumed render enters with the window's batches).  Every such loop of the library, the C++ and
 * Python faces and mcpt_render asks this one function, so they issue the same calls:
 *   *rounds == 0 and *n_passes == 0: finished (done >= max_passes);
 *   *rounds > 0: a queued run of that many rounds of `batch` passes from pass first + done on
 *     (mcpt_adaptive_run* with this check_every).  Only with queued_rounds > 0 and calls a multiple of
 *     check_every: min(queued_rounds, the whole batches left, MCPT_ADAPTIVE_RUN_MAX_ROUNDS) rounds,
 *     trimmed to a multiple of check_every unless the run ends exactly at the cap;
 *   else *n_passes = min(batch, max_passes - done) passes in one mcpt_render_adaptive, followed by a
 *     select iff *select != 0.
 * The caller stops early when a select's record has no active block or a run reports rounds_run
 * below its rounds.  No context and no device: plain host arithmetic.  MCPT_ERR_INVALID_ARG for a
 * non-positive batch, max_passes or check_every, a negative done, calls or queued_rounds, or a NULL
 * out pointer. */
extern int mcpt_adaptive_until_next(int done, int calls, int batch, int max_passes, int check_every, int queued_rounds,
                                    int* rounds, int* n_passes, int* select);

/* Temporal reprojection: carry the integrated frame across camera moves of a
 * static scene.  A context in temporal mode keeps, per pixel of a full frame, the integrated colour,
 * the variance of its mean, the history length and the guides of the frame the history was made with
 * (104 B per pixel; 72 B when the guides are copied, MCPT_TEMPORAL_COPY=1).  Per camera k a caller
 * runs: mcpt_clear_accum, mcpt_stats_begin, two or more mcpt_render batches (first_pass advancing
 * across frames), mcpt_convergence, mcpt_render_guides(camera k), mcpt_temporal_accumulate(P·V of
 * camera k-1), mcpt_denoise_temporal, mcpt_read_denoised.
 *
 * mcpt_temporal_begin: needs a target (else MCPT_ERR_NO_TARGET); allocates the history on the first
 * call and marks it empty (on every call).  Asynchronous.  mcpt_temporal_end: mode off, buffers freed.
 * mcpt_set_target* and mcpt_destroy end the mode; mcpt_upload_scene, mcpt_upload_meshes and
 * mcpt_set_flat_face leave it on and mark the history empty; the accumulator, statistics and render
 * calls do not touch the history.  With the mode off the other calls here return
 * MCPT_ERR_NO_TEMPORAL and no other call does any work for it.
 *
 * mcpt_temporal_accumulate: for every pixel the current colour accum / (float)pass_count and the
 * variance min(se^2, 2^60) of the held error map; its world position through prevPV16 (the FORWARD
 * matrix P·V of the camera the history was made with, column-major: mcpt_mat4_inverse of that
 * camera's invPV) gives a position in the previous frame, whose 2x2 history taps count when they
 * show the same primitive key, lie within plane_tol * dist of the pixel's tangent plane and have a
 * normal within N·Nq >= 0.875.  A pixel with surviving taps blends their bilinear mean h with weight
 * 1 - 1/L, L = min(shortest tap history + 1, max_history): rgb = (1 - 1/L) h + c / L, variance =
 * (1 - 1/L)^2 h.v + v / L^2; every other pixel starts over at {c, v}, length 1.  The history then
 * holds the result and the current guides.  Preconditions, in this order, a refusal changing
 * nothing: the mode on (else MCPT_ERR_NO_TEMPORAL); max_history in 1..65535, positive finite
 * plane_tol, prevPV16 non-NULL unless the history is empty, a full-frame target in row order that
 * holds passes, no gathered count plane, no retired adaptive block (else MCPT_ERR_INVALID_ARG); an
 * error map, the gathered plane when valid else the own window's (else MCPT_ERR_NO_STATS); current
 * guides (else MCPT_ERR_NO_GUIDES).  Asynchronous up to one wait for the record.
 *
 * mcpt_denoise_temporal: the variance filter (mcpt_denoise_variance's iterations, unchanged) from the
 * temporal image, first input {rgb, the 3x3 key-aware prefilter of its variance}.  Needs, in this
 * order: the mode on; iterations in 0..8, positive finite k_color and sigma_plane (else
 * MCPT_ERR_INVALID_ARG); an accumulate since the history was last empty (else MCPT_ERR_NO_STATS);
 * current guides (else MCPT_ERR_NO_GUIDES).  Its result is a variance filter's: mcpt_read_denoised,
 * mcpt_read_denoised_variance and the mcpt_*denoise*_ms / _path queries serve it.  On a first frame
 * it gives mcpt_denoise_variance's bits. */
#define MCPT_TEMPORAL_MAX_HISTORY 65535
typedef struct mcpt_temporal_t {
  long long n_px;
  long long n_history;    /* pixels that blended a history in */
  long long n_new;        /* = n_px - n_history = n_miss + n_offscreen + n_rejected */
  long long n_miss;       /* no primary hit (key < 0) */
  long long n_offscreen;  /* behind the previous camera or outside its frame */
  long long n_rejected;   /* no tap survived (on an empty history: every pixel with a hit) */
  long long sum_len;      /* of the new history lengths */
  int max_len;
  long long frames;       /* accumulates since the history was last empty, this one included */
} mcpt_temporal_t;
int mcpt_temporal_begin(mcpt_ctx* ctx);
int mcpt_temporal_end(mcpt_ctx* ctx);
int mcpt_temporal_accumulate(mcpt_ctx* ctx, const float* prevPV16, int max_history, float plane_tol,
                             mcpt_temporal_t* out);
int mcpt_denoise_temporal(mcpt_ctx* ctx, int iterations, float k_color, float sigma_plane);
/* the history: rgbv4 n x 4 f32 {rgb, variance}, history_len n i32 (either NULL); MCPT_ERR_NO_STATS
 * while the history is empty.  Synchronizes. */
int mcpt_read_temporal(mcpt_ctx* ctx, float* rgbv4, int* history_len);
int mcpt_temporal_info(mcpt_ctx* ctx, int* on, int* history_valid, long long* frames);
/* device ms of the last accumulate: its kernel, and the guides' copy behind it (0 in the ping-pong
 * form); either NULL */
int mcpt_last_temporal_ms(mcpt_ctx* ctx, float* accumulate_ms, float* copy_ms);

/* Temporal adaptive sampling (no reference equivalent): render only the blocks
 * the history cannot carry.  A stopping rule that asks whether the blend this frame's accumulate
 * would write NOW meets the target, and an accumulate that accepts the per-pixel counts this leaves
 * behind.  Per camera k a caller runs:
 *   1. mcpt_clear_accum, mcpt_stats_begin, mcpt_adaptive_begin(min_passes).  mcpt_adaptive_begin on a
 *      context whose mode is on re-initialises the state: every flag set, every block's passes 0,
 *      p0 = the accumulator's pass count (0 after the clear), the list full.
 *   2. mcpt_render_guides(camera k): the rule reads the guides of the camera being rendered.
 *   3. rounds of mcpt_render_adaptive with mcpt_adaptive_select_temporal from the second batch on, or
 *      one mcpt_adaptive_run_temporal.
 *   4. mcpt_temporal_accumulate_resolved(P·V of camera k-1).
 *   5. mcpt_denoise_temporal, mcpt_read_denoised.
 *
 * mcpt_temporal_accumulate_resolved: mcpt_temporal_accumulate with two inputs changed.  The current
 * colour is c = accum / (float)count per channel, mcpt_read_resolved's bits, the count the adaptive
 * mode's (p0 plus the block's passes); the variance is v = min(se^2, 2^60) of the held error map,
 * where retired blocks keep the entries they retired with (as mcpt_denoise_resolved_variance reads
 * them).  The look-up, the tap tests, the blend, the record and both history forms are unchanged.
 * Preconditions: mcpt_temporal_accumulate's, in its order, except that the adaptive mode must be on
 * (else MCPT_ERR_NO_ADAPTIVE, checked right after MCPT_ERR_NO_TEMPORAL) and retired blocks are
 * allowed; a gathered count plane is still refused.  With no block retired it gives
 * mcpt_temporal_accumulate's bits.  mcpt_temporal_accumulate itself still refuses a frame with a
 * retired block.
 *
 * mcpt_adaptive_select_temporal: the third rule behind the select step (beside mcpt_adaptive_select
 * and mcpt_adaptive_select_filtered).  One call, two steps on the context's stream:
 *   A  as mcpt_adaptive_select_filtered's step A: the {se, r} of the active blocks' pixels into the
 *      error map and the raw record; no block retires.
 *   T  for every in-frame pixel of a block that is active on entry, `out` = what
 *      mcpt_temporal_accumulate_resolved(prevPV16, max_history, plane_tol) would write for it now (the
 *      same arithmetic on the history's current set and the map step A wrote; nothing is written to
 *      the history), then in binary32 without contraction in the order written:
 *        Yt = (0.2126 out.r + 0.7152 out.g) + 0.0722 out.b;
 *        rt = sqrt(out.v) / (max(0, Yt) + mu_floor);  rt = 64 if Yt is not finite or not rt <= 64.
 *      The block stays active iff its largest rt > threshold or it holds fewer than min_passes
 *      passes.  Retired blocks are not computed and never return.  The list is rebuilt as
 *      mcpt_adaptive_select rebuilds it.
 * On an empty history every pixel is new, so the rule is a raw-error rule on {c, v}.
 * The record: `raw` as mcpt_adaptive_select_filtered's raw, n_active_blocks = the blocks THIS rule
 * keeps; the other fields run over the in-frame pixels of the blocks active on entry.  Integer sums
 * and a maximum: the bits do not depend on the order.
 * Preconditions, in this order, a refusal changing nothing: adaptive mode on (else
 * MCPT_ERR_NO_ADAPTIVE); temporal mode on (else MCPT_ERR_NO_TEMPORAL); threshold, mu_floor and
 * plane_tol positive and finite, max_history in 1..65535, prevPV16 non-NULL unless the history is
 * empty, a full-frame target in row order that holds passes, no gathered count plane or gathered
 * error map (else MCPT_ERR_INVALID_ARG); statistics on with two batches or more (else
 * MCPT_ERR_NO_STATS); current guides (else MCPT_ERR_NO_GUIDES).
 * mcpt_last_adaptive_ms's select time covers steps A and T with the list scan.  The three selects
 * may alternate freely: all only retire.  Device memory: the filtered select's block of partial
 * records (4 KiB, the statistics buffers' lifetime) serves step T; nothing per pixel.  Synchronizes
 * once, at the end, for the record.
 *
 * mcpt_adaptive_run_temporal: the queued form, mcpt_adaptive_run with this rule (its contract and
 * preconditions as stated there, the select's as above), records of mcpt_adaptive_temporal_t. */
typedef struct mcpt_adaptive_temporal_t {
  mcpt_adaptive_t raw;        /* as mcpt_adaptive_select_filtered's raw: n_active_blocks = what THIS rule keeps */
  long long n_px_t;           /* in-frame pixels of the blocks active on entry */
  long long n_above_t;        /* of those, rt > threshold */
  unsigned long long sum_qt;  /* sum of trunc(rt * 65536) over them */
  float max_rt;
  double mean_rt;             /* sum_qt / 65536 / n_px_t (0 when n_px_t = 0) */
  long long n_history;        /* of those, pixels whose dry-run class is HISTORY */
} mcpt_adaptive_temporal_t;
extern int mcpt_temporal_accumulate_resolved(mcpt_ctx* ctx, const float* prevPV16, int max_history, float plane_tol,
                                             mcpt_temporal_t* out);
extern int mcpt_adaptive_select_temporal(mcpt_ctx* ctx, const float* prevPV16, int max_history, float plane_tol,
                                         float threshold, float mu_floor, mcpt_adaptive_temporal_t* out);
extern int mcpt_adaptive_run_temporal(mcpt_ctx* ctx, const float* invPV, const float* invV, int first_pass, int n_passes,
                                      int rounds, int check_every, float threshold, float mu_floor,
                                      const float* prevPV16, int max_history, float plane_tol, float date, int bounces,
                                      float refract_ind, int variant, mcpt_adaptive_temporal_t* records,
                                      int records_capacity, mcpt_adaptive_run_t* out);

/* DrawSampling's point cloud (DrawSampling/draw_sampling.cpp:144-150, tp/sampling_base.vert
 * seeding, tp/hsphere.vert random_ray): point k = random_ray(normalize(normal), roughness)
 * with seed floatBitsToUint(fseed) + k * nb_used * (11, 43, 67).  out: n × 3 f32 (host). */
int mcpt_sample_hemisphere(mcpt_ctx* ctx, const float* normal3, const float* fseed3, float roughness,
                           int nb_used, int n, float* out_xyz);

/* Use an external hipStream_t (e.g. torch's current stream); NULL = library stream. */
int mcpt_set_stream(mcpt_ctx* ctx, void* hip_stream);
int mcpt_synchronize(mcpt_ctx* ctx);

/* Device time (ms) of the kernel(s) of the last mcpt_render, from HIP events recorded
 * on the launch stream around the launch.  Synchronizes on the end event. */
int mcpt_last_render_ms(mcpt_ctx* ctx, float* ms);
/* The same interval split into the path-tracing kernel and the chunk-combine kernel
 * (launches spanning more than one 32-pass accumulation chunk). */
int mcpt_last_kernel_ms(mcpt_ctx* ctx, float* trace_ms, float* combine_ms);
/* The same for the render call `back` calls before the last (0: the last).  A context keeps the
 * events of its last 64 calls, so a caller can queue a run of calls and read their times
 * afterwards without waiting after each (waits for that call only). */
int mcpt_kernel_ms_back(mcpt_ctx* ctx, int back, float* trace_ms, float* combine_ms);
/* The path-tracing kernel's whole span (its own start on its stream -> its end), summed over the
 * call's sub-launches, for the call `back` calls before the last (waits for it).  With render lanes
 * (mcpt_set_render_lanes) consecutive launches overlap, and mcpt_kernel_ms_back charges each its
 * period (from the previous launch's render end); the span also counts the overlapped tail, as a
 * profiler's kernel duration does. */
int mcpt_kernel_span_ms_back(mcpt_ctx* ctx, int back, float* span_ms);

/* ---------------------------------------------------------------------------------
 * 2. host scene producer (BVH_GPU_Scene-compatible)
 *    material[7] = { r, g, b, a(opacity), shininess, roughness, emissivity }
 *    (Material, bvh_gpu/scene.h:30-49; Material::light(col,e) = {col, 0, 0, e})
 * --------------------------------------------------------------------------------- */
int mcpt_scene_create(mcpt_scene** out);
int mcpt_scene_destroy(mcpt_scene* s);
int mcpt_scene_clear(mcpt_scene* s);                                            /* gpu_bvh_scene.cpp:76-85 */
int mcpt_scene_add_sphere(mcpt_scene* s, const float* trf16, const float* material7);   /* scene.h:128-133 */
int mcpt_scene_add_cube(mcpt_scene* s, const float* trf16, const float* material7);     /* scene.h:135-142 */
int mcpt_scene_add_cylinder(mcpt_scene* s, const float* trf16, const float* material7); /* scene.h:144-152 */
int mcpt_scene_add_cone(mcpt_scene* s, const float* trf16, const float* material7);     /* scene.h:154-163 */
int mcpt_scene_add_oriented_quad(mcpt_scene* s, const float* trf16, const float* material7); /* scene.h:166-172 */
/* Triangle meshes (BVH_GPU_Scene::add_mesh / place_mesh, gpu_bvh_scene.cpp:51-74,
 * gpu_bvh_scene.h:89-92; ScenePrimitives::add_mesh scene.cpp:56-67).  add_mesh stores a mesh
 * (n_vertices × 3 positions and normals, n_triangles × 3 vertex indices) and builds its own
 * median-split BVH over the triangles (SceneMesh::prim_bb); bb6 = the Mesh::BB() box
 * (min.xyz, max.xyz), NULL = the vertices' bounding box.  place_mesh adds an instance (a
 * CODE_MESH primitive) with transform trf and a material, like the reference. */
int mcpt_scene_add_mesh(mcpt_scene* s, const float* vertices, const float* normals, int n_vertices,
                        const unsigned* tri_indices, int n_triangles, const float* bb6, int* mesh_id);
int mcpt_scene_place_mesh(mcpt_scene* s, int mesh_id, const float* trf16, const float* material7);
/* sizes and flat buffers of all meshes, in the layouts mcpt_upload_meshes takes:
 *   info   : n_meshes × 4 i32 (first node, first leaf, BVH depth, first triangle)
 *   nodes  : n_nodes × 6 f32 (bbmin, bbmax; mesh space)   leaves : n_leaves i32 (triangle or -1)
 *   tris   : n_tris × 3 i32 global vertex ids             verts, normals : n_verts × 3 f32 */
int mcpt_scene_mesh_sizes(mcpt_scene* s, int* n_meshes, int* n_nodes, int* n_leaves, int* n_tris, int* n_verts);
int mcpt_scene_get_mesh_buffers(mcpt_scene* s, int* info, float* nodes, int* leaves, int* tris, float* verts,
                                float* normals);
/* Same-topology update of mesh mesh_id (no reference equivalent): replaces its vertices and normals
 * (n_vertices must be the mesh's count, else MCPT_ERR_INVALID_ARG) and refits its BVH boxes; the
 * triangles, the depth and the leaves are kept.  Every leaf gets its triangle's box, a -1 leaf its
 * sibling's, the internal boxes are merged bottom-up as add_mesh merges them: an update with the
 * mesh's own vertices leaves mcpt_scene_get_mesh_buffers bit-identical.  Every new vertex must lie
 * inside the Mesh::BB() the mesh was added with (pass a roomy bb6 to add_mesh for a mesh that will
 * move): the instances' scene-level boxes are trf · BB, and geometry outside would be clipped
 * silently — MCPT_ERR_BAD_SCENE then, and nothing changes.  The scene stays finalized; its prims,
 * nodes and leaves are untouched.  This is the specification of mcpt_refit_mesh. */
int mcpt_scene_update_mesh(mcpt_scene* s, int mesh_id, const float* vertices, const float* normals, int n_vertices);
/* Rebuild of mesh mesh_id's tree from its current vertices (no reference equivalent; DESIGN.md
 * §3.12).  tris == NULL keeps the triangles; otherwise n_tris x 3 mesh-local vertex indices replace
 * them (n_tris must be the mesh's count and every index below its vertex count, else
 * MCPT_ERR_INVALID_ARG and nothing changes), so every buffer size and the depth stay.  The leaves
 * come from a builder with add_mesh's shape (depth, mid = (lo + hi) / 2, axes x, y, z in turn over
 * depth - 1 rounds) and a defined order: `order` starts 0 .. n-1 and every round stable-sorts each
 * of its ranges by the triangle boxes' centre on the round's axis (float `<`; equal keys, -0 and +0
 * among them, keep their order); range s of the last round gives leaves 2s and 2s + 1 (the second
 * -1 for a range of one).  With pairwise distinct keys every internal node holds the triangles
 * add_mesh's tree holds there.  The boxes are then written as mcpt_scene_update_mesh writes them.
 * A mesh of depth 0 has no order: only its triangle row and box follow `tris`.  Mesh::BB() and the
 * instances' boxes do not move; the scene stays finalized.  MCPT_ERR_INVALID_ARG for an unknown
 * mesh.  This is the specification of mcpt_rebuild_mesh. */
int mcpt_scene_rebuild_mesh(mcpt_scene* s, int mesh_id, const unsigned* tris, int n_tris);
/* mesh mesh_id's range in the flat verts / normals arrays of mcpt_scene_get_mesh_buffers */
int mcpt_scene_mesh_vertex_range(mcpt_scene* s, int mesh_id, int* first_vertex, int* n_vertices);
/* sortEmissiveFirst + BVH_KDtree::compute (scene.cpp:70-88, bvh.cpp:34-93) */
int mcpt_scene_finalize(mcpt_scene* s);
int mcpt_scene_nb_prim(mcpt_scene* s, int* n);
int mcpt_scene_depth(mcpt_scene* s, int* depth);
int mcpt_scene_nb_emissives(mcpt_scene* s, int* n);
/* copy the finalized buffers in the layouts mcpt_upload_scene takes */
int mcpt_scene_get_buffers(mcpt_scene* s, float* prims, float* nodes, int* leaves);
/* overwrite (shininess, roughness, emissivity) and colour of finalized prim i (BVH unchanged;
 * emissivity must keep its sign class: the emissive-first order is fixed at finalize) */
int mcpt_scene_set_material(mcpt_scene* s, int prim, const float* material7);
/* the 8 scene builders of MontecarloGPU/montecarlo.cpp:629-795 (keys Q,W,E,R,T,Y,U,I = 1..8),
 * with light_intensity_ (default 1.2, montecarlo.cpp:138).  Clears, builds, finalizes. */
int mcpt_scene_build_reference(mcpt_scene* s, int scene_id, float light_intensity);

/* canonical camera at aspect W/H: fov 0.78, scene radius 145, frame identity,
 * view = modelview · rotateX(-80); outputs (P·V)^-1 and V^-1, column-major */
int mcpt_camera_canonical(int W, int H, float* invPV16, float* invV16);

/* ---------------------------------------------------------------------------------
 * 3. host helpers: Transfo (easycppogl/gl_eigen.cpp:29-105, degrees, column-major) and
 *    the output step
 * --------------------------------------------------------------------------------- */
int mcpt_transfo_translate(float x, float y, float z, float* out16);           /* Transfo::translate */
int mcpt_transfo_scale(float x, float y, float z, float* out16);               /* Transfo::scale */
int mcpt_transfo_rotate(int axis, float degrees, float* out16);                /* rotateX/Y/Z: axis 0/1/2 */
int mcpt_mat4_mul(const float* a16, const float* b16, float* out16);           /* GLMat4 a * b */
/* a^-1 computed in double (cofactors) and rounded to f32; MCPT_ERR_INVALID_ARG for a singular or
 * non-finite matrix.  Turns a camera's invPV into the P·V mcpt_temporal_accumulate takes. */
int mcpt_mat4_inverse(const float* a16, float* out16);
/* fs_frag (montecarlo.cpp:59-70): out = accum / pass_count, per channel */
int mcpt_average(const float* accum, long long n_values, int pass_count, float* out);
/* averaged image (H rows × W × RGB f32, row 0 = bottom) to a little-endian PFM */
int mcpt_write_pfm(const char* path, const float* rgb, int W, int H);
/* what the 8-bit default framebuffer shows: clamp to [0,1], round(255·c), no gamma; PNG RGB8 */
int mcpt_write_png(const char* path, const float* rgb, int W, int H);

/* Checkpoint / resume of a progressive render: the reference's pass loop
 * (montecarlo.cpp:454-466) accumulates into one framebuffer for as long as the window stays
 * open; here a long render (C5: 84,000 passes) can stop and continue in another process with
 * the same bits, because a pass's samples depend only on (pixel, pass, date) and the
 * accumulator is additive.  A file holds the accumulator sums (rows × W × RGB f32, as
 * mcpt_read_accum returns them), the passes they hold, the first pass of the next render call,
 * a caller tag (scene and render parameters) that the reader compares, and the target's
 * identity: the image height H and a hash of the context's image row ids (so a shard's
 * checkpoint cannot be loaded into another shard or another frame of the same local size).
 * Layout, little endian: "MCPTCKP2", int32 W, rows, pass_count, next_pass, tag bytes, H, uint64
 * row-list hash, the tag, then the floats (H = hash = 0: no identity).  The write goes to a
 * temporary file unique to the writer, is flushed to the device (fsync) and renamed over
 * `path`, so an interrupted write or a host crash leaves the previous checkpoint intact.
 * A resumed render equals the uninterrupted one bit for bit when its calls split the pass range
 * at the same points (a call adds its own partial sum of a 32-pass chunk: DESIGN.md §3.3), e.g.
 * the same --chunk in mcpt_render, or call boundaries on multiples of 32 passes. */
#define MCPT_CHECKPOINT_TAG_MAX 1024
/* The context's accumulator, pass count, `next_pass`, `tag` (may be NULL) and target identity.
 * Synchronizes the context's stream. */
int mcpt_checkpoint_save(mcpt_ctx* ctx, const char* path, int next_pass, const char* tag);
/* Resume: loads a file written by mcpt_checkpoint_save for THIS target (W, local rows, H and
 * row ids must match; MCPT_ERR_INVALID_ARG otherwise, and for a file without identity) and,
 * when `tag` is not NULL, with this tag; sets the accumulator and pass count and returns the
 * next call's first pass in *next_pass (may be NULL). */
int mcpt_checkpoint_load(mcpt_ctx* ctx, const char* path, const char* tag, int* next_pass);
/* File-level access without a context (no target identity: H = hash = 0). */
int mcpt_checkpoint_write(const char* path, const float* rgb, int W, int rows, int pass_count, int next_pass,
                          const char* tag);
/* Reads the header into W, rows, pass_count, next_pass (any may be NULL) and the tag into tag_out
 * (MCPT_CHECKPOINT_TAG_MAX bytes, NUL-terminated; may be NULL); the sums into rgb_out
 * (rows × W × 3 floats, at most `capacity` floats) unless it is NULL.  MCPT_ERR_INVALID_ARG for
 * a missing, foreign or truncated file, or sums larger than `capacity`.  Reads "MCPTCKP1" files
 * (round 3, no identity) too. */
int mcpt_checkpoint_read(const char* path, float* rgb_out, long long capacity, int* W, int* rows, int* pass_count,
                         int* next_pass, char* tag_out);

/* Checkpoint / resume of an ADAPTIVE render: the accumulator together with the
 * statistics window, the error map and the blocks' state, so that a long adaptive render can stop
 * and continue.  The guarantee: after mcpt_adaptive_checkpoint_load the same sequence of
 * mcpt_render_adaptive / mcpt_adaptive_select calls produces the same records, active lists, error
 * maps, sample counts and sums, bit for bit, as the uninterrupted render.
 * Layout, little endian, no padding: "MCPTCKA1"; int32 W, rows, pass_count, next_pass, tag bytes, H;
 * uint64 row-list hash; int32 p0 (the pass count at mcpt_adaptive_begin), min_passes; int64 passes
 * and int32 batches of the statistics window; int32 1 if the error map is valid; int32 n_blocks,
 * blocks_x; the tag; per block the active flag (n_blocks int32), then the passes (n_blocks int32);
 * per pixel the accumulator (rows x W x 3 f32), the statistics state {Yacc, S2, Ybase, 0} (x 4
 * f32) and the error map {se, r} (x 2 f32).  Written as mcpt_checkpoint_write writes (temporary
 * file unique to the writer, fsync, rename, directory fsync).  The two formats do not cross-load:
 * mcpt_checkpoint_read / _load return MCPT_ERR_INVALID_ARG for an "MCPTCKA1" file and the adaptive
 * reader and loader for an "MCPTCKP1/2" file. */
typedef struct mcpt_adaptive_checkpoint_t {
  int W, rows, pass_count, next_pass, H;
  unsigned long long rows_hash;   /* H = rows_hash = 0: no target identity */
  int p0, min_passes;
  long long stats_passes;
  int stats_batches, emap_valid;
  int n_blocks, blocks_x;         /* ceil(W / 8) * ceil(rows / 8), ceil(W / 8) */
} mcpt_adaptive_checkpoint_t;
/* Needs the adaptive mode on (else MCPT_ERR_NO_ADAPTIVE).  Synchronizes the context's stream. */
extern int mcpt_adaptive_checkpoint_save(mcpt_ctx* ctx, const char* path, int next_pass, const char* tag);
/* Loads a file written by mcpt_adaptive_checkpoint_save for THIS target (W, local rows, H and row
 * ids must match, and `tag` when it is not NULL; MCPT_ERR_INVALID_ARG otherwise, with
 * mcpt_checkpoint_load's details): sets the accumulator and pass count, turns statistics and the
 * adaptive mode on in the saved state (their buffers as mcpt_stats_begin / mcpt_adaptive_begin
 * allocate them, the active list rebuilt from the flags) and returns the next call's first pass in
 * *next_pass (may be NULL).  Synchronizes. */
extern int mcpt_adaptive_checkpoint_load(mcpt_ctx* ctx, const char* path, const char* tag, int* next_pass);
/* File-level access without a context, plain arrays: block_active and block_passes hold
 * hdr->n_blocks ints, accum / stats4 / emap2 hold rows x W x 3 / 4 / 2 floats.  The header must be
 * consistent (positive sizes, n_blocks and blocks_x of W x rows), else MCPT_ERR_INVALID_ARG. */
extern int mcpt_adaptive_checkpoint_write(const char* path, const mcpt_adaptive_checkpoint_t* hdr, const char* tag,
                                   const int* block_active, const int* block_passes, const float* accum,
                                   const float* stats4, const float* emap2);
/* Reads the header into *hdr (may be NULL) and the tag into tag_out (MCPT_CHECKPOINT_TAG_MAX bytes;
 * may be NULL).  The five arrays are read when all are given (all NULL: header only): at most
 * block_capacity blocks and pixel_capacity pixels.  MCPT_ERR_INVALID_ARG for a missing, foreign or
 * truncated file (the file's length must be the one its header implies), an inconsistent header,
 * or arrays larger than the capacities. */
extern int mcpt_adaptive_checkpoint_read(const char* path, mcpt_adaptive_checkpoint_t* hdr, char* tag_out, int* block_active,
                                  int* block_passes, long long block_capacity, float* accum, float* stats4,
                                  float* emap2, long long pixel_capacity);

#ifdef __cplusplus
}
#endif

#endif /* MCPT_H_ */
