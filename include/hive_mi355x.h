/*
 * hive_mi355x.h -- C ABI of libhive_mi355x.so: the MI355X (gfx950) implementation of HIVE's
 * per-frame dense-compute path (depth-map -> TSDF volume fusion, view frusta, depth-to-point
 * unprojection / projection, mask dilation, marching cubes, DPT ViT blocks).
 *
 * HIVE itself has no FFI: its boundary for this path is a set of plain Python call
 * signatures.  Every entry point below cites the reference call site
 * (file:line under /root/reference) whose arithmetic it replaces; INTEGRATION.md shows
 * the ctypes binding a HIVE maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (HIVE_OK) or a negative hive_status; the message for the
 *     last failure on a context is returned by hive_last_error(ctx) (ctx may be NULL for
 *     failures of hive_ctx_create itself: thread-local).
 *   - plain pointers and sizes only; `mem` says whether image/point pointers are host
 *     (HIVE_MEM_HOST: copied through a pinned staging buffer, the call returns after the
 *     copy so the caller may overwrite its arrays -- hive/fusion.py:121 mutates depth_im
 *     right before integrate) or device memory (HIVE_MEM_DEVICE: used in place, stream
 *     ordered on the context's stream).
 *   - one hive_ctx per (GPU, stream); contexts are independent, so Python threads may own
 *     separate contexts (the reference calls the geometric functions from a ThreadPool,
 *     hive/pipeline.py:491).  A single context is not re-entrant.
 *   - volumes are three float32 arrays [X][Y][Z] (z fastest), as in the reference library:
 *     tsdf (init 1), weight (init 0), colour packed b*65536 + g*256 + r (init 0).
 *   - there is no CPU fallback: every compute entry point needs a gfx950 device.
 */
#ifndef HIVE_MI355X_H
#define HIVE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIVE_ABI_VERSION 9

typedef enum hive_status {
    HIVE_OK = 0,
    HIVE_ERR_INVALID = -1,   /* bad argument (shape, NULL, size)                 */
    HIVE_ERR_DEVICE = -2,    /* HIP runtime failure; message has the hipError_t  */
    HIVE_ERR_NOMEM = -3,     /* device / pinned allocation failed                */
    HIVE_ERR_EMPTY = -4,     /* no surface: tsdf has no zero crossing (the reference raises
                                ValueError there, scripts/experiments.py:165-168) */
    HIVE_ERR_STATE = -5      /* call sequence error (e.g. copy_mesh before extract) */
} hive_status;

typedef enum hive_mem_kind { HIVE_MEM_HOST = 0, HIVE_MEM_DEVICE = 1 } hive_mem_kind;

/* Rounding of real-valued pixel coordinates / colours to integers.
 * HALF_EVEN = numpy's np.round (the reference library's CPU path and hive/geometric.py:176);
 * HALF_AWAY = C roundf (the reference library's CUDA kernel).  SURVEY.md §7(b). */
typedef enum hive_round_mode { HIVE_ROUND_HALF_EVEN = 0, HIVE_ROUND_HALF_AWAY = 1 } hive_round_mode;

typedef struct hive_ctx hive_ctx;
typedef struct hive_tsdf hive_tsdf;

/* ---- library / context ------------------------------------------------------------ */
int hive_abi_version(void);
/* `stream` is the hipStream_t every kernel and copy of the context is issued on, e.g.
 * torch.cuda.current_stream().cuda_stream.  NULL is HIP's default (null) stream -- which is what that
 * expression returns for PyTorch's default stream -- and HIVE_STREAM_OWN makes the context create a
 * non-blocking stream of its own. */
#define HIVE_STREAM_OWN ((void *)(intptr_t)-1)
/* ... and HIVE_STREAM_OWN_LOW one of the LOWEST dispatch priority (hipStreamCreateWithPriority): for work that should fill what the
 * other streams leave idle -- the TSDF sweeps of a batch under the next batch's network (hive_amd.depth.DepthFusionStream(overlap=True)). */
#define HIVE_STREAM_OWN_LOW ((void *)(intptr_t)-2)
int hive_ctx_create(int device_id, void *stream, hive_ctx **out);
int hive_ctx_destroy(hive_ctx *ctx);
/* The hipStream_t the context issues on (e.g. to wrap a context-owned stream in torch.cuda.ExternalStream). */
int hive_ctx_get_stream(hive_ctx *ctx, void **stream);
int hive_ctx_synchronize(hive_ctx *ctx);
const char *hive_last_error(hive_ctx *ctx);
/* Give up ownership of a private stream (HIVE_STREAM_OWN / _OWN_LOW): hive_ctx_destroy will then NOT destroy it.  For callers that hand the stream to a
 * framework which keeps referring to it after the context is gone -- PyTorch's caching allocator records an event on every stream a tensor was used on
 * (`Tensor.record_stream`) when the tensor is freed, possibly long after the context died, and process groups cache streams too; recording on a destroyed
 * stream crashes the process (found by tests/test_distributed_gpu.py::test_rccl_merge_of_a_volume_on_the_overlap_side_stream).  The Python binding calls
 * this as soon as it wraps the stream for torch (`Context.torch_stream()`): such a stream lives until the process ends. */
int hive_ctx_release_stream(hive_ctx *ctx);
/* Re-binds the context to another hipStream_t (NULL = the default stream).  The new stream is ordered behind
 * everything already queued on the old one.  The Python binding calls this when torch's current stream changes
 * (e.g. inside `with torch.cuda.stream(s)`), so that hive kernels stay ordered with the surrounding torch ops. */
int hive_ctx_set_stream(hive_ctx *ctx, void *stream);
/* Rounding used by hive_project / hive_project_bbox, and the mode a volume created afterwards on this context starts with. */
int hive_ctx_set_round_mode(hive_ctx *ctx, int mode);
/* Deterministic mode (off by default): the network kernels stop using the three paths whose USE depends on the batch size and on the device's CU count --
 * split-K of long K loops at small launches (another, fixed, order of float32 additions), the attention kernel's two-way split of the keys at small grids
 * (likewise) and the Gram-matrix form of the GroupNorm statistics of the bottlenecks' 1 x 1 convolutions (statistics of the exact products instead of the
 * rounded outputs) -- so that a frame's depth map no longer changes
 * with the size of the batch it was in beyond what is stated next.  What remains: a GroupNorm's per-tile partial sums are cut at 128- / 256-pixel
 * tile boundaries counted from the START OF THE BATCH, so a frame's (mean, rstd) still depend on its position in the batch by float32 re-association
 * (~1e-7 relative).  Frame-sharded multi-GPU runs that want one-GPU depth maps to the last bit must also keep the per-rank batch composition. */
int hive_ctx_set_deterministic(hive_ctx *ctx, int enabled);
/* Launch counters of the small-launch paths since creation (or the last call with reset != 0): GEMM / convolution launches that split their K loop,
 * and launches of the four-stage-ring kernels (csrc/mfma_pipe.hpp).  Diagnostic: the one-frame parity tests assert with it that those paths ran. */
int hive_ctx_launch_stats(hive_ctx *ctx, int64_t *splitk_launches, int64_t *deep_ring_launches, int reset);
/* HIP-event timing of the most recent kernel launched by a *_timed call on this context. */
int hive_ctx_set_timing(hive_ctx *ctx, int enabled);
int hive_ctx_last_kernel_ms(hive_ctx *ctx, float *ms);
/* Sum and count of the HIP-event durations of every dominant-kernel launch (integrate) made on
 * this context since timing was enabled or since the previous call; synchronises the stream. */
int hive_ctx_kernel_time_total(hive_ctx *ctx, int *n_launches, float *total_ms);

/* ---- TSDF volume: replaces third_party/tsdf_fusion_python `fusion.TSDFVolume` ------ */
/* fusion.TSDFVolume(vol_bnds, voxel_size)           -- hive/fusion.py:104
 * vol_bnds is row-major [3][2] = {xmin,xmax, ymin,ymax, zmin,zmax} (float64, as hive/fusion.py:48).
 * vol_dim = ceil((max-min)/voxel_size); origin = float32(min); trunc = 5*voxel_size.
 * If d_tsdf/d_weight/d_color are non-NULL the volume lives in caller-owned device memory
 * (e.g. torch tensors) of vol_dim[0]*vol_dim[1]*vol_dim[2] floats each; otherwise the
 * library allocates.  The volume is initialised (1,0,0) either way. */
int hive_tsdf_dims(const double vol_bnds[6], double voxel_size, int64_t vol_dim[3]);
int hive_tsdf_create(hive_ctx *ctx, const double vol_bnds[6], double voxel_size,
                     float *d_tsdf, float *d_weight, float *d_color, hive_tsdf **out);
/* An x-slab of the same scene grid: the volume holds grid voxels x_begin <= x < x_end (all y, z), dims (x_end - x_begin, Y, Z),
 * and every voxel keeps the world position it has in the whole grid (origin + index * voxel_size with the GRID index, bit for
 * bit) -- so integrating a frame into the slabs of a partition gives exactly the slices of integrating it into the whole
 * volume.  For the bit-exact multi-GPU mode (frames all-gathered, volume sharded in x-slabs).  x_end < 0 = the
 * whole grid.  hive_tsdf_info reports the slab's dims and the grid's origin / bounds; extract_mesh needs a whole volume. */
int hive_tsdf_create_slab(hive_ctx *ctx, const double vol_bnds[6], double voxel_size, int64_t x_begin, int64_t x_end,
                          float *d_tsdf, float *d_weight, float *d_color, hive_tsdf **out);
int hive_tsdf_slab_info(hive_tsdf *vol, int64_t *x_begin, int64_t *grid_dim_x);
int hive_tsdf_destroy(hive_tsdf *vol);
/* Rounding of THIS volume's pixel projection and colour average (integrate, accum_finalize): the reference library has two
 * arithmetic paths -- its CUDA kernel rounds with roundf (HIVE_ROUND_HALF_AWAY; what `TSDFVolume(..., use_gpu=True)` runs when
 * pycuda is installed, as in the reference's Docker image, requirements.txt:14) and its numpy path with np.round
 * (HIVE_ROUND_HALF_EVEN; `use_gpu=False`, BASELINE config 1). */
int hive_tsdf_set_round_mode(hive_tsdf *vol, int mode);
int hive_tsdf_reset(hive_tsdf *vol);
/* Tell the library that the caller wrote the volume's planes itself (caller-owned storage of hive_tsdf_create): cached mesh results
 * and the fast paths that rely on what the library knows about the planes' contents (every weight a whole number of unit
 * observations since the last reset -- the division-free colour update of the sweep) are dropped until the next hive_tsdf_reset. */
int hive_tsdf_planes_modified(hive_tsdf *vol);
int hive_tsdf_info(hive_tsdf *vol, int64_t vol_dim[3], float origin[3], double vol_bnds[6],
                   float *voxel_size, float *trunc_margin);
/* device pointers of the three volumes (for RCCL collectives / zero-copy views) */
int hive_tsdf_device_ptrs(hive_tsdf *vol, float **d_tsdf, float **d_weight, float **d_color);

/* TSDFVolume.integrate(color_im, depth_im, cam_intr, cam_pose, obs_weight) -- hive/fusion.py:124
 * color u8 [H][W][3] RGB, depth f32 [H][W] metres (0 = invalid), K f32 row-major 3x3,
 * cam_pose f64 row-major 4x4 camera-to-world.  n_updated (optional, host) receives the number
 * of voxels written by this call (forces a stream sync).
 * Depths that are not positive finite numbers get no special treatment: a voxel in front of the camera that rounds to a pixel is
 * updated unless `depth == 0` or `depth - cam_z < -trunc` -- the contract's tests, evaluated in float32 as the CPU oracle evaluates
 * them.  So -0.0 is invalid like 0; a negative depth d updates the voxels with 0 < cam_z <= trunc + d (dist < 0);
 * +inf and NaN update EVERY voxel in front of the camera that rounds to the pixel, with dist = 1 (`diff < -trunc` is false for a NaN, and
 * fminf(1, NaN) = 1).  Callers that want such pixels ignored set them to 0 first. */
int hive_tsdf_integrate(hive_tsdf *vol, const uint8_t *color, const float *depth, int H, int W,
                        const float K[9], const double cam_pose[16], float obs_weight,
                        int mem, uint64_t *n_updated);
/* n frames back to back (frame f at color + f*H*W*3, depth + f*H*W, poses + f*16), in order:
 * identical results (bit for bit) to n calls of hive_tsdf_integrate.  Device-resident frames are swept up to four
 * consecutive frames per launch: a voxel is loaded once, the frames are applied to it in order, it is stored once. */
int hive_tsdf_integrate_batch(hive_tsdf *vol, int n, const uint8_t *color, const float *depth,
                              int H, int W, const float K[9], const double *cam_poses,
                              float obs_weight, int mem);
/* How the most recent hive_tsdf_integrate_batch on this volume grouped its frames: *n_groups launches, sizes[i] frames in
 * sweep i (1 = the single-frame kernel), in order; at most `capacity` sizes are written.  Diagnostic: the parity tests assert
 * with it that the fused sweep really ran (the semantics are those of hive/fusion.py:113-124's serial loop either way). */
int hive_tsdf_last_batch_groups(hive_tsdf *vol, int *sizes, int capacity, int *n_groups);
/* Length of the work list the most recent sweep on this volume ran over (segments of *segment_voxels consecutive z voxels
 * that survive the per-row frustum / depth clip); forces a stream sync.  Diagnostic: n_items * segment_voxels against the voxels
 * a sweep updates is the share of its arithmetic that can change a voxel (bench.py reports it). */
int hive_tsdf_last_sweep_items(hive_tsdf *vol, uint64_t *n_items, int *segment_voxels);
/* What the volume has been given since its creation / last hive_tsdf_reset: frames handed to integrate / integrate_batch /
 * accum_integrate (`frames`) and the integrate launches that applied them (`launches`: one per single-frame kernel, one per fused
 * sweep).  Host-side bookkeeping, no stream sync.  bench.py prints it next to the weight plane's sum as the timed job's proof of work
 * (one TSDFVolume.integrate call of hive/fusion.py:124 = one frame here). */
int hive_tsdf_stats(hive_tsdf *vol, int64_t *frames, int64_t *launches);
/* TSDFVolume.get_volume(): copies tsdf and colour (and weight) out (any may be NULL).  The destinations / sources of
 * get_volume / set_volume may be host OR device memory (unified addressing decides the copy direction). */
int hive_tsdf_get_volume(hive_tsdf *vol, float *h_tsdf, float *h_color, float *h_weight);
int hive_tsdf_set_volume(hive_tsdf *vol, const float *h_tsdf, const float *h_color, const float *h_weight);
/* Overwrite voxels [first, first + count) of the three planes from device (or host) arrays of `count` floats each (any may be
 * NULL): how the pieces of an all-gather (a rank's share of the merged volume, or an x-slab) are put in place. */
int hive_tsdf_set_volume_range(hive_tsdf *vol, int64_t first, int64_t count, const float *d_tsdf, const float *d_weight, const float *d_color);

/* TSDFVolume.get_mesh() -- hive/fusion.py:127.  Two steps because the sizes are data dependent:
 * extract counts and builds the mesh on the device, copy_mesh copies it out.
 * verts f32 [nv][3] world coordinates, faces i32 [nf][3], norms f32 [nv][3], colors u8 [nv][3] (RGB).
 * Vertex order: ascending (voxel linear index, axis); face order: ascending cell linear index,
 * then table order.  Returns HIVE_ERR_EMPTY when there is no zero crossing. */
int hive_tsdf_extract_mesh(hive_tsdf *vol, int64_t *n_verts, int64_t *n_faces);
int hive_tsdf_copy_mesh(hive_tsdf *vol, float *verts, int32_t *faces, float *norms, uint8_t *colors);
/* vertices of the same extraction in voxel units (before x voxel_size + origin), f32 [nv][3] */
int hive_tsdf_copy_mesh_voxel_coords(hive_tsdf *vol, float *verts_vox);

/* Alternative to accum_integrate for a rank that fused its own frames with hive_tsdf_integrate: convert its
 * running-average volumes into the same sums, planes = [tsdf * w, w, r * w, g * w, b * w], ready for the all-reduce.
 * (The per-rank colours are already rounded per frame, so the merged colour can differ from the sequential one by the
 * same +-2 levels as with accum_integrate; tsdf and weight merge exactly up to float re-association.) */
int hive_tsdf_accum_from_volume(hive_tsdf *vol, float *d_accum);
/* The same sums laid out for ONE reduce-scatter over `world` ranks: d_out is float [world][5][chunk]; voxel i goes to piece
 * i / chunk, offset i % chunk (world * chunk >= N; the tail past N is written as zeros).  Rank r's reduce-scatter output is then
 * its [5][chunk] share, the input of hive_tsdf_accum_finalize_to with plane_stride = chunk. */
int hive_tsdf_accum_from_volume_sharded(hive_tsdf *vol, float *d_out, int world, int64_t chunk);
/* Frame-sharded fusion (BASELINE.json north_star): a rank accumulates
 * num = sum(w_i*dist_i), w = sum(w_i), rgb = sum(w_i*c_i) for its frames into 5 float planes
 * [5][X][Y][Z]; planes are summed across ranks (RCCL all-reduce by the caller), then folded
 * into the volume.  d_accum must hold 5*N floats of device memory, zeroed by accum_reset. */
int hive_tsdf_accum_reset(hive_tsdf *vol, float *d_accum);
int hive_tsdf_accum_integrate(hive_tsdf *vol, float *d_accum, const uint8_t *color, const float *depth,
                              int H, int W, const float K[9], const double cam_pose[16],
                              float obs_weight, int mem);
int hive_tsdf_accum_finalize(hive_tsdf *vol, const float *d_accum);
/* The same arithmetic (and the volume's round mode) for `count` voxels of 5 planes of `plane_stride` floats each, into explicit
 * device arrays d_tsdf / d_weight / d_color [count]: what a rank runs on ITS share of the voxels after a reduce-scatter of the
 * planes; the three result arrays are then all-gathered (hive_amd.distributed.fuse_sharded). */
int hive_tsdf_accum_finalize_to(hive_tsdf *vol, const float *d_accum, int64_t plane_stride, int64_t count, float *d_tsdf,
                                float *d_weight, float *d_color);

/* ---- Sparse merge: only the observed voxel SEGMENTS go through the collectives (hive_amd.distributed.fuse_sharded(merge="sparse")) ------
 * A segment is a run of L consecutive voxels of the linear C-order index (z fastest): segment s = [s * L, min((s + 1) * L, N)),
 * S = ceil(N / L) segments; L is a power of two in 64 .. 4096.  A segment is INACTIVE iff every weight word in it has the bit pattern of
 * +0.0f (the bits decide, not w == 0: a -0.0f is active and goes through the same arithmetic as in the dense merge); everything else is active.
 * Contract: a voxel of weight +0.0f holds the initial values (tsdf 1, colour 0).  That is true of every volume the integrate kernels produce,
 * and it is what hive_tsdf_accum_finalize_to writes for w == 0, so leaving an inactive segment untouched equals what the dense merge writes there.
 * All arrays are device memory; every offset is 64-bit. */
/* d_flags u8 [S]: 1 for an active segment, 0 for an inactive one.  Reads the weight plane once (4 N bytes); one byte store per segment. */
int hive_tsdf_mark_segments(hive_tsdf *vol, int L, uint8_t *d_flags);
/* The same for a bare weight plane of n floats: plane 1 of raw accumulator planes [5][n] (d_accum + n). */
int hive_mark_segments(hive_ctx *ctx, const float *d_weight, int64_t n, int L, uint8_t *d_flags);
/* d_list i32 [S] (room for every segment): the indices of the segments whose flag is non-zero, ascending, at [0, *d_count); the rest of d_list
 * is not written.  d_count is ONE int64 in device memory: the caller's 8-byte copy of it to the host is the only synchronisation the sparse
 * merge adds. */
int hive_segment_list(hive_ctx *ctx, const uint8_t *d_flags, int64_t n_segments, int32_t *d_list, int64_t *d_count);
/* The five sums [tsdf * w, w, r * w, g * w, b * w] (the expressions of hive_tsdf_accum_from_volume_sharded) of the n_active listed segments
 * laid out for ONE reduce-scatter over `world` ranks: d_out is float [world][5][per * L] with per >= ceil(n_active / world); list entry k goes
 * to piece k / per, floats [(k % per) * L, (k % per + 1) * L) of each of that piece's planes, so piece r holds the active segments
 * [r * per, min((r + 1) * per, n_active)).  Everything past n_active, and the lanes past N in the volume's last segment, are written as
 * zeros.  Rank r's reduce-scatter output is its [5][per * L] share: the input of hive_tsdf_accum_finalize_to with plane_stride = per * L and
 * count = (its number of segments) * L.  n_active == 0 returns HIVE_OK without a launch. */
int hive_tsdf_accum_from_volume_segments(hive_tsdf *vol, const int32_t *d_list, int64_t n_active, int L, int world, int64_t per, float *d_out);
/* The same layout from raw accumulator planes d_accum [5][n] (hive_tsdf_accum_integrate): a plain gather of the 5 planes. */
int hive_accum_pack_segments(hive_ctx *ctx, const float *d_accum, int64_t n, const int32_t *d_list, int64_t n_active, int L, int world, int64_t per,
                             float *d_out);
/* The way back: d_in is float [world][3][per * L] (tsdf, weight, colour: the all-gathered shares, laid out as above with 3 planes per
 * piece); the n_active listed segments are written into the volume's planes, never past N, and no other voxel is touched.  Drops the cached
 * mesh and the volume's unit-weight fast path, as hive_tsdf_set_volume_range does.  n_active == 0 returns HIVE_OK without a launch. */
int hive_tsdf_set_volume_segments(hive_tsdf *vol, const int32_t *d_list, int64_t n_active, int L, int world, int64_t per, const float *d_in);

/* ---- fusion.get_view_frustum(depth_im, cam_intr, cam_pose) -- hive/fusion.py:59 ------ */
/* out: float64 row-major [3][5] (apex + 4 corners at max(depth)), world coordinates */
int hive_view_frustum(hive_ctx *ctx, const float *depth, int H, int W, const float K[9],
                      const double cam_pose[16], int mem, double out[15]);

/* The bounds pass of adjust_voxel_size (hive/fusion.py:53-61) for a whole frame set at once: n depth maps [n][H][W] (already in HBM
 * when mem = HIVE_MEM_DEVICE), poses f64 [n][16] -> out f64 [n][3][5]; ONE reduction launch and ONE read-back of n maxima instead
 * of n launches + n synchronisations.  Same values as n calls of hive_view_frustum. */
int hive_view_frustum_batch(hive_ctx *ctx, const float *depth, int n, int H, int W, const float K[9],
                            const double *cam_poses, int mem, double *out);

/* ---- hive/geometric.py ------------------------------------------------------------- */
/* point_cloud_from_depth(depth, mask, K, R, t)  -- hive/geometric.py:107-126 (+ image2world :183-206)
 * valid = mask & (depth > 0); points in row-major (v,u) order; X = R^T (d * Kinv [u,v,1]^T - t).
 * Kinv = np.linalg.inv(K) evaluated by the caller in K's dtype (geometric.py:203) and widened to f64.
 * mask u8 [H][W] (non-zero = keep; NULL = all), R f64[9], t f64[3] (world-to-camera),
 * out_xyz f64 [capacity][3] (host or device per `mem`), *n = number of points written.
 * rgb (optional u8 [H][W][3]) / out_rgba (u8 [capacity][4], alpha 255): point_cloud_from_rgbd :129-152 */
int hive_unproject(hive_ctx *ctx, const float *depth, const uint8_t *mask, const uint8_t *rgb,
                   int H, int W, const double Kinv[9], const double R[9], const double t[3],
                   int mem, double *out_xyz, uint8_t *out_rgba, int64_t capacity, int64_t *n);
/* image2world(points, depth, K, R, t, scale_factor) -- hive/geometric.py:183-206, for an explicit
 * list of pixel coordinates: uv f64 [n][2], depth f64 [n] -> out_xyz f64 [n][3] */
int hive_image2world(hive_ctx *ctx, const double *uv, const double *depth, int64_t n, const double Kinv[9],
                     const double R[9], const double t[3], double scale_factor, int mem, double *out_xyz);
/* world2image(points, K, R, t, scale_factor, dtype) -- hive/geometric.py:155-180
 * points f64 [n][3]; out_uv_i32 (rounded per ctx round mode, default half-even = np.round) or
 * out_uv_f64 (exactly one non-NULL); out_depth f64 [n] */
int hive_project(hive_ctx *ctx, const double *points, int64_t n, const double K[9], const double R[9],
                 const double t[3], double scale_factor, int mem,
                 int32_t *out_uv_i32, double *out_uv_f64, double *out_depth);

/* world2image + the visibility reduction of HiveDataset.select_key_frames -- hive/io.py:1161-1175:
 * project points (f64 [n][3]), rounded per the context's round mode (default half-even = np.round), keep pixels inside [0,W) x [0,H) and return
 * out = {min u, max u, min v, max v, count} (count == 0: the extrema are INT_MAX / INT_MIN). */
int hive_project_bbox(hive_ctx *ctx, const double *points, int64_t n, const double K[9], const double R[9],
                      const double t[3], int W, int H, int mem, int32_t out[5]);

/* ---- foreground per-frame meshes: Pipeline._create_scene's inner loops -- hive/pipeline.py:340-483 ------------------ */
/* _triangulate_faces (:651-667) + _filter_faces (:670-694) in one pass over the frame: the valid pixels (mask & depth > 0) of
 * a depth map are a lattice, so the triangulation is the implicit one of the pixel grid (two triangles per fully valid 2 x 2
 * block, one per block with three valid corners) and only faces whose edges are all <= max_pixel_distance pixels long and span
 * <= max_depth_distance metres are emitted (hive/options.py:271-286: defaults 2 and 0.1).  out_faces i32 [capacity][3] index the
 * rows of hive_unproject's output for the same depth / mask (valid pixels in row-major order), wound like the reference's
 * reversed Delaunay simplices; face order: row-major by block.  *n_faces = number of faces found (may exceed capacity: call
 * with capacity 0 to size the buffer); *n_vertices (optional) = number of valid pixels. */
int hive_grid_mesh(hive_ctx *ctx, const float *depth, const uint8_t *mask, int H, int W, double max_pixel_distance,
                   double max_depth_distance, int mem, int32_t *out_faces, int64_t capacity, int64_t *n_faces,
                   int64_t *n_vertices);
/* One object of one frame in ONE call (the body of process_frame's loop, hive/pipeline.py:383-461, without the CPU-library stages between -- decimation, connected
 * components, billboard): point_cloud_from_depth (:386; hive_unproject's rows) -> _triangulate_faces + _filter_faces (:402-408; hive_grid_mesh's faces) ->
 * _get_mesh_texture_and_uv (:453; hive_texture_window's uv and crop box), everything device-resident: d_depth f32 [H][W], d_mask u8 [H][W] (NULL = all pixels) in;
 * d_vertices f64 [vertex_capacity][3], d_faces i32 [face_capacity][3], d_uv i32 [vertex_capacity][2] out (H W and 4 H W are always enough).  Kinv = inverse
 * intrinsics as the caller computes it (numpy.linalg.inv, as hive/geometric.py:201), K, R, t the camera as for hive_unproject / hive_project.  Seven launches and
 * ONE read-back (through pinned memory): *n_vertices, *n_faces, bbox = {min_u, min_v, max_u + 1, max_v + 1} (the texture is image[min_v:max_v, min_u:max_u]).
 * Results are bit-identical to the three separate entry points on the same inputs. */
int hive_fg_frame_mesh(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, const double Kinv[9], const double K[9], const double R[9],
                       const double t[3], double max_pixel_distance, double max_depth_distance, double *d_vertices, int64_t vertex_capacity, int32_t *d_faces,
                       int64_t face_capacity, int32_t *d_uv, int64_t *n_vertices, int64_t *n_faces, int32_t bbox[4]);
/* _cleanup_with_connected_components (:741-779, trimesh 3.9's face_adjacency + graph.connected_components): two faces are adjacent when they share an
 * edge (unordered vertex pair) that exactly two faces use; a face without an adjacent face belongs to no component and is always removed; a component
 * survives with at least min_len faces; is_object != 0 keeps only the largest survivor (on a tie the one whose smallest face index is smallest), 0 keeps
 * all of them.  Survivors keep their order.  Vertices: those at least one INPUT face references (Trimesh(process=True) drops the others before any face
 * goes), in input order -- out_vertex_index i32 [n_vertices_out] lists their input ids, out_faces i32 [n_faces_out][3] index that list (no merging of
 * coincident vertices, so the result equals trimesh's up to vertex order).  Without faces every vertex is kept.  faces i32 [n_faces][3] with ids in
 * [0, n_vertices), n_vertices < 2^30, n_faces < 2^29; out_faces room for n_faces rows, out_vertex_index for n_vertices; mem = where all three live. */
int hive_mesh_cleanup_cc(hive_ctx *ctx, const int32_t *faces, int64_t n_faces, int64_t n_vertices, int is_object, double min_len, int mem,
                         int32_t *out_faces, int32_t *out_vertex_index, int64_t *n_faces_out, int64_t *n_vertices_out);
/* hive_fg_frame_mesh with the clean-up above between the face filter and the texture window (pipeline.py:402-453 with decimation off): the faces that
 * survive hive_mesh_cleanup_cc(is_object, min_len) in d_faces, the vertices the filtered faces reference in d_vertices (renumbered in row-major pixel
 * order), uv and bbox over those vertices.  before (optional) = {valid pixels, faces after the filter}: the counts the reference tests before the
 * clean-up (pipeline.py:388, 410).  Same buffers and one read-back; H W < 2^27.  hive_fg_frame_mesh itself is unchanged. */
int hive_fg_frame_mesh_cc(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, const double Kinv[9], const double K[9], const double R[9],
                          const double t[3], double max_pixel_distance, double max_depth_distance, int is_object, double min_len, double *d_vertices,
                          int64_t vertex_capacity, int32_t *d_faces, int64_t face_capacity, int32_t *d_uv, int64_t *n_vertices, int64_t *n_faces, int32_t bbox[4],
                          int64_t before[2]);
/* _decimate_mesh (:697-738: OpenMesh's ModQuadric with set_max_err(max_error), binary mode, and decimate_to_faces(budget)) as a parallel halfedge collapse.
 * The rules of this build (OpenMesh's ModQuadricT / BaseDecimaterT as published; not compared with OpenMesh itself):
 *   quadrics   per face (p0, p1, p2) in float64: n = (p1 - p0) x (p2 - p0), area = |n|; if area > FLT_MIN: n /= area, area *= 0.5; d = -(p0 . n);
 *              Q = area [n d]^T [n d] (10 terms); each vertex sums the quadrics of its faces in ascending face index.  Q(v1) += Q(v0) after a collapse;
 *              quadrics are never rebuilt from the current faces.
 *   collapse   halfedge v0 -> v1: v0 goes, its faces take v1; no position moves, so the output vertices are input rows bit for bit.  Cost = (Q(v0) +
 *              Q(v1))(p1), legal only if cost < max_error; priority = (float)cost.
 *   topology   legal only if: the common neighbours of v0 and v1 are exactly the edge's opposite vertices (link condition); a boundary v0 collapses only
 *              along a boundary edge onto a boundary v1; two boundary vertices joined by an interior edge do not collapse; for each opposite vertex the
 *              edges to v0 and v1 are not both boundary edges; not (vl, vr adjacent and both of valence 3); v0 has at least two faces; v1 has at
 *              most 24 faces afterwards (faces(v0) + faces(v1) - faces removed <= 24: a rule of this build that keeps fans small).
 *   locked     vertices with a number of boundary edges other than 0 or 2 (bowties), and the ends of edges with more than two faces, take part in no
 *              collapse (a rule of this build: OpenMesh's add_face on such input is not reproduced).
 *   rounds     every unlocked vertex picks its cheapest legal collapse on the mesh at the start of the round (ties: smallest v1); its key is the cost's
 *              band (the top 5 of the order-preserving float32 bits: 16 octaves) << 32 | mix32(v0) (a bijective hash: unique keys, in random order
 *              within a band -- exact cost order leaves few local minima, so few collapses per round); a collapse is
 *              applied iff its key is the smallest within two edges of v0 and within two edges of v1 -- applied collapses share no face.  When they
 *              would remove at least F - budget faces only the cheapest prefix by key that reaches F <= budget is applied.
 *   stop       at F <= budget (a reachable budget ends at budget or budget - 1) or when no legal collapse is left; budget >= F returns the input.  More
 *              than 4096 rounds with legal collapses left: HIVE_ERR_STATE.
 * Output: the surviving vertices in input order, isolated ones included (out_vertex_index i32 [n_vertices_out] = their input ids), the surviving faces in
 * input order indexing them (out_faces i32 [n_faces_out][3]).  stats (may be NULL) = {rounds, collapses, locked vertices}, all 0 when budget >= F.
 * vertices f64 [n_vertices][3], faces i32 [n_faces][3] with ids in [0, n_vertices) and no repeated id in a face (else HIVE_ERR_INVALID); n_vertices
 * < 2^30, n_faces < 2^29, budget >= 0; out_faces room for n_faces rows, out_vertex_index for n_vertices; mem = where all four live.  Deterministic. */
int hive_mesh_decimate(hive_ctx *ctx, const double *vertices, int64_t n_vertices, const int32_t *faces, int64_t n_faces, int64_t budget, double max_error, int mem,
                       int32_t *out_faces, int32_t *out_vertex_index, int64_t *n_faces_out, int64_t *n_vertices_out, int64_t stats[3]);
/* The reference's per-object order (pipeline.py:402-453): hive_fg_frame_mesh's triangulation + face filter, hive_mesh_decimate(budget, max_error), with
 * enable_cc the clean-up of hive_fg_frame_mesh_cc(is_object, min_len), then the texture window over the vertices left.  d_vertices: the vertices that
 * survive (all the decimation keeps -- isolated ones included -- or, with the clean-up, those its faces reference), in row-major pixel order; d_faces
 * index them.  before (optional) = {valid pixels, faces after the filter}, decimated (optional) = {vertices, faces} after the decimation, stats as
 * hive_mesh_decimate's.  Same buffers as hive_fg_frame_mesh; besides the final read-back, one small read-back per batch of 16 decimation rounds
 * decides whether to go on.  H W < 2^27.  hive_fg_frame_mesh and hive_fg_frame_mesh_cc are unchanged. */
int hive_fg_frame_mesh_dec(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int H, int W, const double Kinv[9], const double K[9], const double R[9],
                           const double t[3], double max_pixel_distance, double max_depth_distance, int64_t budget, double max_error, int enable_cc,
                           int is_object, double min_len, double *d_vertices, int64_t vertex_capacity, int32_t *d_faces, int64_t face_capacity, int32_t *d_uv,
                           int64_t *n_vertices, int64_t *n_faces, int32_t bbox[4], int64_t before[2], int64_t decimated[2], int64_t stats[3]);
/* _filter_faces (:670-694) for an explicit face list of any triangulation: points2d i32 [n][2] (u, v), depth f32 [n], faces i32
 * [F][3] -> the faces whose three edges pass both limits, order preserved, into out_faces (capacity F). */
int hive_filter_faces(hive_ctx *ctx, const int32_t *points2d, const float *depth, int64_t n_points, const int32_t *faces,
                      int64_t n_faces_in, double max_pixel_distance, double max_depth_distance, int mem, int32_t *out_faces,
                      int64_t *n_faces_out);
/* _get_mesh_texture_and_uv (:782-808): uv = world2image(vertices) in its default int32 form (np.round); bbox = {min_u, min_v,
 * max_u + 1, max_v + 1} -- the crop `image[min_v:max_v, min_u:max_u]` that becomes the texture; out_uv i32 [n][2] = uv - (min_u, min_v). */
int hive_texture_window(hive_ctx *ctx, const double *points, int64_t n, const double K[9], const double R[9], const double t[3],
                        double scale_factor, int mem, int32_t *out_uv, int32_t bbox[4]);
/* Billboard (hive/pipeline.py:439-447): `c = rotation @ (vertices.T + translation); c[2, :] = np.median(c[2, :]); vertices = (rotation.T @ (c - translation)).T`
 * in place on d_vertices f64 [n][3] (device).  The map is the reference's R (p + t) and back R^T (c - t), NOT hive_project's R p + t: for t != 0 the two are not
 * inverses of each other, and this is restated as it stands.  Operation order (no fused multiply-add): c_r = (R[r][0] (x + t0) + R[r][1] (y + t1)) + R[r][2] (z + t2);
 * out_j = (R[0][j] (c_0 - t0) + R[1][j] (c_1 - t1)) + R[2][j] (m - t2).  m is numpy's median EXACTLY (middle order statistic for odd n, (a + b) / 2 of the two
 * middle ones for even n): a radix select over the order-preserving 64-bit image of the doubles, 8 bits a pass, integer histograms across workgroups -- the same
 * bits whatever the launch shape; -0 sorts before +0; finite values only.  *median_out (optional, host) = m, at the price of one synchronisation; n = 0: no-op.
 * Follow with hive_texture_window on the flattened vertices (:449-453). */
int hive_fg_billboard(hive_ctx *ctx, double *d_vertices, int64_t n, const double R[9], const double t[3], double *median_out);
/* Centroids of the dynamic objects for ForegroundPoseOptimiser (hive/pose_optimisation.py:1626-1634, 1654-1657): out_centroids[i] = mean, in camera space, of
 * point_cloud_from_depth(depth_i, mask_i > 0, K) and out_counts[i] = its length, for n_frames <= 65535 device-resident frames d_depth f32 [n][H][W], d_mask u8
 * [n][H][W] (instance ids, non-zero = object); no point cloud is materialised.  Per point hive_unproject's arithmetic with R = I, t = 0; float64 sums in a fixed tree
 * that depends on H W alone (tiles of 4096 pixels: 16 per thread in order, lane butterfly, waves in order; then the tiles likewise), so the result is bit-identical
 * from run to run.  out_centroids f64 [n][3] and out_counts i64 [n] are host arrays; a frame without a valid object pixel has count 0 and centroid 0. */
int hive_fg_centroids(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_frames, int H, int W, const double Kinv[9], double *out_centroids,
                      int64_t *out_counts);
/* The Adam loop of ForegroundPoseOptimiser.run (hive/pose_optimisation.py:1669-1709), all num_epochs epochs in ONE launch of one workgroup.  params f64 [n][7] =
 * (scalar-last quaternion, translation) in / out (host): the raw parameters, not normalised.  gt_params (NULL = params): the parameters the fixed world-space
 * centroids gt = conj(q / |q|) (c - t) are taken at -- the reference takes them at the initial parameters.  centroids f64 [n][3] (hive_fg_centroids); chunks: n_chunks
 * runs [chunk_start[c], chunk_start[c] + chunk_len[c]) of at least 3 frames, ascending and disjoint.  Per epoch and chunk, with w = conj(q / |q|) (c - t):
 * 0.01 mean_i |gt_i - w_i| + 0.1 |t[:-2] - 2 t[1:-1] + t[2:]|_F + 0.1 |t[:-1] - t[1:]|_F, summed over the chunks; hand-derived gradients (0 where a norm is 0, as
 * torch.norm's); torch.optim.Adam(lr = learning_rate, weight_decay = 1e-4) semantics on every parameter, frames of no chunk included.  losses f64 [num_epochs + 1]:
 * the loss before every epoch's step and, last, at the returned parameters.  gradient (optional) f64 [n][7]: dL/dparams at the returned parameters, without the
 * weight decay (with num_epochs = 0: loss and gradient at `params`).  Float64 throughout -- the reference keeps the parameters in float32 --, fixed summation
 * order: bit-identical from run to run. */
int hive_fts_optimise(hive_ctx *ctx, double *params, const double *gt_params, const double *centroids, int n_frames, const int32_t *chunk_start,
                      const int32_t *chunk_len, int n_chunks, double learning_rate, int num_epochs, double *losses, double *gradient);

/* ---- PoseOptimiser._optimisation_loop (hive/pose_optimisation.py:1256-1519) as PROJECTED Adam -- csrc/poseopt.hip */
typedef enum hive_pose_alignment { HIVE_POSE_RIGID = 0, HIVE_POSE_AFFINE = 1, HIVE_POSE_DEFORMABLE = 2 } hive_pose_alignment;
typedef enum hive_pose_residual { HIVE_POSE_WORLD3D = 0, HIVE_POSE_IMAGE2D = 1 } hive_pose_residual;
typedef struct hive_pose_options {
    int32_t num_epochs, lr_scheduler_patience, early_stopping_patience;
    int32_t alignment_type, residual_type; /* hive_pose_alignment, hive_pose_residual */
    int32_t smooth_trajectory, position_only;
    int32_t reserved;
    double learning_rate, l2_regularisation, min_loss_delta, pose_t_reg, pose_r_reg;
} hive_pose_options;
/* The Adam loop over the camera poses p_f = (q_f scalar-last, t_f), world-to-camera, and -- Affine -- a depth scale and shift per frame, against the M
 * correspondences of a FeatureSet.  DELIBERATE DEVIATION, not pinned against the reference's run: the reference assigns new Parameter objects for the normalised
 * quaternions and the clipped positions every epoch while its optimiser keeps the old ones, so its step() moves nothing; this is the intent, projected Adam --
 * every epoch normalises the quaternions and clips the positions IN PLACE and Adam then steps those same parameters, moments and step count carried through.
 * Float64 parameters and arithmetic (the reference: float32), no contraction, every sum in an order fixed by the problem: bit-identical from run to run and for
 * every check_every.
 *   params f64 [n][7] in / out (host): raw, the returned ones as the last step left them (not normalised).  scale, shift f64 [n] in / out (host; Affine, else NULL).
 *   d_index_{i,j} i64 [M], d_points_{i,j} f32 [M][2] (u, v), d_depth_{i,j} f32 [M]: DEVICE arrays, the tensors of a FeatureSet.
 * One epoch e, with lr_e decided after the loss of epoch e - 1 (lr_0 = learning_rate):
 *   1. q_f := q_f / sqrt(((x^2 + y^2) + z^2) + w^2), component by component.
 *   2. if max_frame_distance >= 0 (= clip_distance / fps; negative: no clip): d_f = t_f - t_{f-1} of the positions as they are; |d_f| = sqrt((dx^2 + dy^2) + dz^2); where
 *      |d_f| > max_frame_distance, d_f := (max_frame_distance / |d_f|) d_f; frames before the first such f stay as they are, from it on t_f := t_{f-1} + d_f, frame after
 *      frame (shifting all later frames by a correction, as the reference does, leaves later differences untouched).
 *   3. loss = (sum_f share_f) -- the shares added thread k taking frames k, k + 256, .., lane butterfly xor 32 .. 1, four waves in order -- where share_f =
 *      (sum over the correspondences with index_i = f of |r_k|) / M + the regulariser terms whose FIRST frame is f, and, per correspondence, with u = q / |q|:
 *        camera point c = (((u - c_x) * depth) / f_x, ((v - c_y) * depth) / f_y, depth) -- Rigid: computed once; Affine: depth = 1 / (scale_f (1 / depth) + shift_f);
 *        World3D: r = p - q, p = conj(u_i) (c_i - t_i) u_i, q likewise on side j;   Image2D: x = u_j p conj(u_j) + t_j, r = (u_j, v_j) - ((f_x x + c_x z) / z,
 *        (f_y y + c_y z) / z), no guard on z;
 *      smooth_trajectory: + pose_t_reg (mean_a |t_a - t_{a+1}|^2 + mean_a |D2_a|^2 + mean_a |D2_a - D2_{a+1}|^2), D2_a = (t_a - 2 t_{a+1}) + t_{a+2}, + pose_r_reg
 *      mean_a (1 - (q_a . q_{a+1})^2) on the raw quaternions; a mean over no rows (n < 4) is 0, not NaN;   Affine: + l2 mean_f (1 / scale_f - 1)^2 + 2 l2 mean_f shift_f^2.
 *   4. the gradient by hand (formulas at the top of poseopt.hip; 0 where |r_k| = 0, as torch.norm's): per frame the sum over its incidence list -- every (k, side)
 *      with index_side[k] = f, ascending in k, side i before j -- thread j taking entries j, j + 256, .., lane butterfly, waves in order; then the regularisers; then
 *      frame 0's pose gradient := 0 and, position_only, every quaternion gradient := 0.
 *   5. torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay): m += (1 - b1) (g - m), v = b2 v + (1 - b2) g g, p -= lr_e / (1 - b1^k) * m / (sqrt(v) /
 *      sqrt(1 - b2^k) + eps), b^k by repeated multiplication.
 *   6. ReduceLROnPlateau(mode min, threshold_mode abs, threshold min_loss_delta, patience lr_scheduler_patience, factor 0.1, cooldown 0, min_lr 0, eps 1e-8) on the
 *      loss: better if loss < best - threshold; more than patience bad epochs: lr := 0.1 lr if that lowers it by more than 1e-8, bad count := 0.  Then the
 *      reference's EarlyStopping: improved if loss < best and |loss - best| > min_loss_delta; stop once the calls since the last best exceed
 *      early_stopping_patience.  Both run ON THE DEVICE; after a stop every queued launch is a no-op.  The host enqueues check_every epochs and then reads the state.
 * losses, learning_rates f64 [num_epochs] (host): entries [0, *epochs_run) are written -- the loss of each epoch's projected parameters before its step, and the
 * learning rate after the scheduler saw that loss (what the next epoch uses).  *final_loss, gradient f64 [n][9] (both optional): the loss and d/d(q, t, scale, shift)
 * with the pins applied at the RETURNED parameters, no projection -- with num_epochs = 0, at the input.  Refused with a message: n < 2, M < 1, an index outside
 * [0, n), a depth or focal length that is not positive and finite, Deformable; a loss that is not finite ends the call with an error naming the epoch. */
int hive_pose_optimise(hive_ctx *ctx, double *params, double *scale, double *shift, int n_frames, double fx, double fy, double cx, double cy,
                       const int64_t *d_index_i, const float *d_points_i, const float *d_depth_i, const int64_t *d_index_j, const float *d_points_j,
                       const float *d_depth_j, int64_t n_matches, const hive_pose_options *options, double max_frame_distance, int check_every, double *losses,
                       double *learning_rates, int *epochs_run, double *final_loss, double *gradient);
/* Steps 1 and 2 of an epoch of hive_pose_optimise alone, on params f64 [n][7] in / out (host), n >= 1: what the tests hold against the stated order. */
int hive_pose_project(hive_ctx *ctx, double *params, int n_frames, double max_frame_distance);

/* ---- motion segmentation: instance masks from the static model (hive_amd/segmentation.py).  The reference takes its masks from detectron2's Mask R-CNN
 * (hive/io.py:163-230), which is absent here; these are rules of this project: they find what moved against the fused model, not persons.  The format is the
 * reference's: u8, 0 = background, 1 .. k = objects, ids per frame and not tracked over time (io.py:214-218).  Everything is batched over n frames
 * [n][H][W] in device memory, 1 <= n <= 65535, H * W < 2^30; nothing synchronises except where it says so.
 * Rule `motion`.  live, model f32, metres, 0 = invalid.  In float32, each operation rounded once, no fused multiply-add:
 *     rel = relative_difference * model;  thr = min_difference > rel ? min_difference : rel;  diff = model - live;
 *     mask = live > 0 && model > 0 && diff > thr            (written 0 / 1)
 *   i.e. the live surface lies more than max(min_difference, relative_difference * model) in front of the model's along the same ray.  A pixel whose ray
 *   found no model surface is not set: unknown, not moving.  Both parameters finite and not negative.
 * Rule `open`.  The set is mask != 0.  `iterations` erosions and then `iterations` dilations with the 3 x 3 square = one (2 it + 1)^2 box minimum and then one
 *   box maximum, each over the pixels of the picture alone: pixels outside take no part (cv2's default border; for the dilation hive_dilate_mask's
 *   convention).  Output 0 / 1.  iterations = 0: out = mask byte for byte.  0 <= iterations <= 16.  d_out may be d_mask.
 * Rule `label`.  The set is mask != 0; two set pixels are neighbours when they differ by one in u or in v (connectivity 4) or by at most one in both
 *   (connectivity 8); a component is a class of the closure of that relation.  A component's root is the smallest raster index v * W + u among its pixels, its
 *   area the number of its pixels.  Components with area < min_area are removed (area == min_area stays); the others are numbered 1 .. k in ascending order of
 *   their roots (the order scipy.ndimage.label numbers them in).  labels = the number of the pixel's component, 0 for clear pixels and removed components;
 *   d_counts[frame] = k; d_areas (may be NULL with area_capacity 0) i32 [n][area_capacity]: the area of component j at j - 1, zeros behind k, components past
 *   the capacity not written.  The result is a function of the mask alone: the order in which workgroups run, and which of two racing unions wins, changes
 *   no bit of it.  label_bytes 4: d_labels i32, any k, no synchronisation.  label_bytes 1: d_labels u8; the call waits for the device and fails with
 *   HIVE_ERR_INVALID, naming the first such frame and its count, when a frame has more than 255 components left (labels and counts are written all the same).
 * hive_motion_segment: `motion`, `open` in place, `label` into u8 ids, in one call; one read-back at its end (the 255 limit). */
int hive_motion_mask(hive_ctx *ctx, const float *d_live, const float *d_model, int n, int H, int W, float min_difference, float relative_difference,
                     uint8_t *d_mask);
int hive_mask_open(hive_ctx *ctx, const uint8_t *d_mask, int n, int H, int W, int iterations, uint8_t *d_out);
int hive_label_components(hive_ctx *ctx, const uint8_t *d_mask, int n, int H, int W, int connectivity, int min_area, int label_bytes, void *d_labels,
                          int32_t *d_counts, int32_t *d_areas, int area_capacity);
int hive_motion_segment(hive_ctx *ctx, const float *d_live, const float *d_model, int n, int H, int W, float min_difference, float relative_difference,
                        int opening_iterations, int connectivity, int min_area, uint8_t *d_ids, int32_t *d_counts);

/* ---- dilate_mask(mask, MaskDilationOptions(num_iterations)) -- hive/image_processing.py:30-45 */
/* 3x3 rectangular structuring element applied `iterations` times == one (2*it+1)^2 box max
 * (cv2.dilate border = no contribution from outside).  mask/out u8 [H][W], non-zero = set; out is written as 0 / 1 and must not
 * overlap mask (both functions). */
int hive_dilate_mask(hive_ctx *ctx, const uint8_t *mask, int H, int W, int iterations, int mem,
                     uint8_t *out);

/* The same with the caller's structuring element (hive/options.py:245-268: `MaskDilationOptions(num_iterations, dilation_filter)`):
 * se u8 [kh][kw] (host memory, 1x1 .. 32x32, non-zero = member, at least one member), cv2.dilate's definition -- anchor at
 * (kw / 2, kh / 2), taps outside the image ignored, the pass repeated `iterations` times (0 = copy).  A full rectangle of odd sides
 * takes the separable box-max path; anything else is iterated literally. */
int hive_dilate_mask_se(hive_ctx *ctx, const uint8_t *mask, int H, int W, const uint8_t *se, int kh, int kw, int iterations, int mem,
                        uint8_t *out);

/* Masking of the depth maps of a frame set on the device (all pointers device memory; d_out may alias d_depth):
 *   mode 0 -- background volume, hive/fusion.py:118-121: `mask = dilate_mask(mask, iterations); depth[mask > 0] = 0`;
 *   mode 1 -- foreground volume (BASELINE config 5: the complement): depth is kept where the UNDILATED mask is set, 0 elsewhere.
 * d_mask u8 [n][H][W] instance ids (hive/io.py:214-218: 0 = background, 1..k = objects); instance_id > 0 restricts "set" to that
 * object, 0 = any object. */
int hive_depth_apply_mask_se(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n, int H, int W, const uint8_t *se, int kh,
                             int kw, int iterations, int mode, int instance_id, float *d_out); /* the same, any structuring element (host) */
int hive_depth_apply_mask(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n, int H, int W, int iterations,
                          int mode, int instance_id, float *d_out);
/* The loader's depth transform on the device (hive/io.py:1032-1039): uint16 millimetres -> float32 metres
 * (`depth_scale * mm`), `> max_depth -> 0`. */
int hive_depth_mm_to_m(hive_ctx *ctx, const uint16_t *d_mm, int64_t n, float depth_scale, float max_depth, float *d_out);

/* ---- inpainting behind the dynamic objects -- DatasetAdaptor._inpaint_frame_data, hive/dataset_adaptors.py:473-571, InpaintingMode.CV2_Image_Depth:
 *      `cv2.inpaint(image, mask, 30, cv2.INPAINT_TELEA)` --------------------------------------------------------------------------------------------
 * cv2's Telea is a sequential, heap-ordered fast-marching pass; its output is not pinned here.  The specification of record is Telea's
 * published method (A. Telea, "An Image Inpainting Technique Based on the Fast Marching Method", 2004, eq. 2-3 and the weight of section 2.3), reordered so that
 * the result does not depend on scheduling, and stated to the bit:
 *
 * Inputs.  image u8 [H][W][C], C = 1 or 3, or u16 [H][W]; mask u8 [H][W], non-zero = hole; integer radius eps, 2 <= eps <= 64; H, W <= 4096.  A frame
 *   without a hole is copied unchanged; a frame without a known pixel is HIVE_ERR_INVALID, and so is eps < 2 (the guarantee below needs the diagonal
 *   neighbours) or eps > 64.
 * Distances.  d_in2(p): the exact squared Euclidean distance (an integer) from hole pixel p to the nearest known pixel; d_out2(q): the same from known
 *   pixel q to the nearest hole pixel.
 * Level set.  T = sqrt(d_in2) on the hole, T = 1 - sqrt(d_out2) outside, float64.
 * Levels.  level(p) = the smallest integer L with L * L >= d_in2(p), in integers; known pixels have level 0.  The hole is filled level by level, L = 1, 2, ...
 *   At level L the USABLE pixels are those of level < L, with their stored values (already rounded to the integer type); pixels of one level never read
 *   each other.  Every hole pixel has an 8-neighbour of lower level (a unit step towards the nearest known pixel shortens the distance by at least 1), which
 *   eps >= 2 puts inside the window: the weight sum is never zero, and the number of fill launches is the largest level.
 * A pixel p = (x, y) of level L.  gT = ((T(x + 1, y) - T(x - 1, y)) / 2, (T(x, y + 1) - T(x, y - 1)) / 2), coordinates clamped to the image.  The window
 *   offsets are indexed k = (dy + eps) (2 eps + 1) + (dx + eps), q = p + (dx, dy); a term exists for 0 < dx^2 + dy^2 <= eps^2, q inside the image, q usable.
 *   With r = p - q = (-dx, -dy) as float64 and r2 = dx^2 + dy^2:
 *     dst = 1 / (r2 * sqrt(r2))
 *     lev = 1 / (1 + |T(q) - T(p)|)
 *     dir = |r.x * gT.x + r.y * gT.y|;  dir <= 0.01 -> dir = 1e-6
 *     w   = (dst * lev) * dir
 *   per channel, gI(q) along x: (I(qx + 1, qy) - I(qx - 1, qy)) / 2 when both neighbours are inside the image and usable, I(qx + 1, qy) - I(q) or
 *   I(q) - I(qx - 1, qy) when one is, 0 when none is; along y likewise;
 *     term = w * (I(q) + (gI.x * r.x + gI.y * r.y))
 * Sums.  64 partial sums: partial j starts at 0.0 and adds the terms (for s: the weights w) of the offsets k = j, j + 64, j + 128, ... in ascending k.
 *   Then v[j] = v[j] + v[j + off] for j < off, off = 32, 16, 8, 4, 2, 1; the sum is v[0].  Ia (per channel) and s are summed alike.
 * Output.  clamp(floor(Ia / s + 0.5), 0, 255 or 65535).  Known pixels are never written.
 * Arithmetic.  float64 IEEE add, subtract, multiply, divide, sqrt; no fused multiply-add.
 * Three things differ from cv2: level order instead of heap order, exact distances instead of the eikonal solve, the paper's gradient term
 * instead of cv2's normalised variant.
 *
 * hive_inpaint_telea: one image, `mem` = HIVE_MEM_HOST or HIVE_MEM_DEVICE for image, mask and out alike; bytes_per_sample 1 (channels 1 or 3) or 2 (channels 1).
 * out may be the image itself (device).  Host calls write nothing to `out` when the frame is refused. */
int hive_inpaint_telea(hive_ctx *ctx, const void *image, int H, int W, int channels, int bytes_per_sample, const uint8_t *mask, int radius, int mem, void *out);
/* The frames of a batch at once, device memory: d_rgb u8 [n][H][W][3], d_depth u16 [n][H][W] (either may be NULL, with its output), d_mask u8 [n][H][W].
 * `d_mask != 0` is first dilated as hive_dilate_mask_se does with a full dilate_kh x dilate_kw element, dilate_iterations times (0 = not at all; the
 * reference: 5 x 5, 5 times).  Colour and depth share the mask, the levels and the weights; the hole pixels of all frames are sorted by (level, frame, y, x)
 * and one launch fills a level of every frame, so a batch costs its largest level count in fill launches.  Bit for bit the frames run one by one, and two
 * hive_inpaint_telea calls per frame.  Outputs may be the inputs.  levels_out (host, optional) i32 [n]: each frame's level count (0 = no hole).
 * n * H * W < 2^31. */
int hive_inpaint_frames(hive_ctx *ctx, const uint8_t *d_rgb, const uint16_t *d_depth, const uint8_t *d_mask, int n, int H, int W, int dilate_kh, int dilate_kw,
                        int dilate_iterations, int radius, uint8_t *d_rgb_out, uint16_t *d_depth_out, int32_t *levels_out);

/* ---- rendering meshes from a camera pose -- render_mesh(camera_matrix, camera_pose, *meshes), scripts/experiments.py:861-883 (pyrender, RenderFlags.FLAT;
 * scored against the frame at :835-852).  An exact z-buffer rasteriser; several meshes share one depth test through four calls on one key plane
 * d_key u64 [H][W]:  hive_render_clear, hive_render_draw per mesh, hive_render_shade per mesh, hive_render_resolve.  The rules (float64, no fused multiply-add):
 *   camera     K, R, t as for hive_project (world-to-camera), the project's camera frame as it stands: x right, y down, z forward.  The reference's
 *              diag(1, -1, -1, 1) only converts to pyrender's OpenGL camera and is not restated.
 *   vertex     hive_project's operation order: cam_r = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t_r; c_r = (K[r][0] cam_0 + K[r][1] cam_1) + K[r][2] cam_2;
 *              sx = c_0 / c_2, sy = c_1 / c_2, z = c_2 (hive_project's depth; the camera-space z for a K whose last row is 0 0 1) -- a vertex lands where
 *              world2image puts it.  Snapped to 8 sub-pixel bits: X = (int)floor(sx * 256 + 0.5), Y likewise.
 *   samples    pixel (i, j) samples the screen point x = j, y = i: world2image's convention (it rounds to the pixel index), not OpenGL's half-pixel offset.  A
 *              mesh built from a frame and rendered from that frame's pose puts every vertex back on its pixel.
 *   rejection  a face is discarded when a vertex has !(z >= near) -- no clipping: triangles here are voxel- or pixel-sized --, when a vertex has
 *              !(|sx| < 65536 && |sy| < 65536) (the guard band keeps every edge function below 2^53: int64 -> double is exact), or when the snapped area
 *              A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) is 0.  near > 0 (0.05 in the Python wrapper); no far plane.
 *   coverage   exact in int64, no back-face culling: A < 0 swaps vertices 1 and 2 and uses |A|.  For the edge opposite vertex e, from p = e + 1 to q = e + 2
 *              (mod 3): w_e = (Xq - Xp)(256 i - Yp) - (Yq - Yp)(256 j - Xp); inside iff for every edge w_e > 0 or (w_e == 0 and (dy < 0 or (dy == 0 and
 *              dx > 0))) -- the top-left rule.  Candidates: the bounding box ceil(min / 256) .. floor(max / 256) clipped to the screen.
 *   depth      q_e = (double)w_e / z_e; den = (q0 + q1) + q2; depth = (float)(1.0 / (den / (double)A)).
 *   visibility key = (uint64)float_bits(depth) << 32 | global face index, and the pixel keeps the MINIMUM key (one 64-bit unsigned atomic minimum): the
 *              nearest surface, on equal float32 depth the smaller face index, whatever the arrival order or the launch shape.  The global face index is
 *              face_base + the face's row: the caller numbers the meshes' faces consecutively in argument order.  An empty pixel holds all ones.
 *   shading    unlit and perspective-correct, as RenderFlags.FLAT: an attribute a is ((q0 a0 + q1 a1) + q2 a2) / den with the edge functions recomputed
 *              from the snapped vertices at the winner.  Vertex colours: each channel (uint8)min(255, floor(c + 0.5)).  Textures: (u, v) in the atlas
 *              convention of Pipeline._pack_textures (u = column / width, v = 1 - row / height), nearest texel col = clamp(floor(u Wt + 0.5), 0, Wt - 1),
 *              row = clamp(floor((1 - v) Ht + 0.5), 0, Ht - 1).  Empty pixels: the background colour, depth 0, face -1.
 * All pointers named d_ are device memory; K, R, t and background are host arrays.  Nothing synchronises. */
/* Every pixel of the key plane to "empty" (all ones): the start of a picture, pyrender's fresh scene at experiments.py:861-883.  H W < 2^31. */
int hive_render_clear(hive_ctx *ctx, uint64_t *d_key, int H, int W);
/* The depth test of one mesh (experiments.py:871-881 adds the meshes to one scene): d_vertices f64 [nv][3], d_faces i32 [nf][3] with ids in [0, nv) (a face with
 * another id is skipped, never read), its faces numbered face_base .. face_base + nf - 1 (< 2^32 - 1).  Scratch of the caller, filled here and read again by
 * hive_render_shade: d_xy i32 [nv][2] the snapped (X, Y) and d_z f64 [nv] the depth of every vertex (0 marks a rejected vertex: a kept one has z >= near > 0);
 * d_large i32 [nf]: the faces whose clipped box holds more than 64 pixels, drawn by one workgroup each (the others by one thread each); d_counts u32 [2] =
 * {faces on that list, faces drawn by their own thread} of this call (faces rejected or off screen are in neither).  nv, nf < 2^31. */
int hive_render_draw(hive_ctx *ctx, const double *d_vertices, int64_t nv, const int32_t *d_faces, int64_t nf, int64_t face_base, const double K[9], const double R[9],
                     const double t[3], int H, int W, double near, int32_t *d_xy, double *d_z, int32_t *d_large, uint32_t *d_counts, uint64_t *d_key);
/* The colour of the pixels whose winner lies in [face_base, face_base + nf) (experiments.py:861-883 renders with RenderFlags.FLAT), after EVERY mesh has been drawn:
 * the same d_faces, nf, face_base, d_xy and d_z as the mesh's hive_render_draw; d_vertex_colors u8 [nv][3], or NULL and d_uv f64 [nv][2] with d_texture
 * u8 [Ht][Wt][3]; d_color u8 [H][W][3].  Other pixels are left alone. */
int hive_render_shade(hive_ctx *ctx, int64_t nv, const int32_t *d_faces, int64_t nf, int64_t face_base, const int32_t *d_xy, const double *d_z,
                      const uint8_t *d_vertex_colors, const double *d_uv, const uint8_t *d_texture, int Ht, int Wt, const uint64_t *d_key, int H, int W,
                      uint8_t *d_color);
/* The planes of the finished picture (experiments.py:847 relies on the white background of :861-883): empty pixels of d_color u8 [H][W][3] (may be NULL) take
 * background[3] (NULL = white); d_depth f32 [H][W] (may be NULL) the winner's depth, 0 where empty; d_face i32 [H][W] (may be NULL) its global face index, -1
 * where empty (an index of 2^31 or more does not fit: keep the total below 2^31 when the face plane is wanted). */
int hive_render_resolve(hive_ctx *ctx, const uint64_t *d_key, int H, int W, const uint8_t background[3], uint8_t *d_color, float *d_depth, int32_t *d_face);

/* ---- texturing a mesh from posed frames (no counterpart in the reference, whose background mesh keeps the volume's vertex colours: pipeline.py:258-286).  Per
 * face the ONE view that sees it best, an atlas with two faces per block, one gather per texel.  The rules (float64, no fused multiply-add, in the order written):
 *   select     once per view, after that view's hive_render_clear / hive_render_draw / hive_render_resolve(depth), on the d_xy and d_z the draw filled (the snap
 *              and the projection are the rasteriser's).  Face f is a candidate iff its three vertices were kept (d_z > 0), its snapped area A (as above) is
 *              not 0, and for every vertex k the nearest pixel (i, j) = ((Y_k + 128) >> 8, (X_k + 128) >> 8) (arithmetic shifts) lies on the screen, has
 *              mask[i][j] == 0, and has depth[i][j] == 0 || z_k <= (double)depth[i][j] + depth_tolerance (a pixel nothing covers hides nothing).
 *              key = |A| << 16 | (65535 - view_index); d_best[f] = max(d_best[f], key): the largest exact snapped area -- the nearest, least oblique view --,
 *              on equal area the lower view index, whatever the order of the calls; 0 = no view.  (|A| < 2^47: the vertices lie within half a pixel of a screen
 *              with (H + 1)(W + 1) <= 2^31.)  LIMITATION: there is no back-face test; a face seen from behind through nothing nearer is a candidate.
 *   layout     faces 2k and 2k + 1 share block k of S x S texels, S = cell in [6, 64].  blocks = ceil(nf / 2), per_row = ceil(sqrt(blocks)),
 *              Wt = per_row S, Ht = ceil(blocks / per_row) S (neither above 16384); block k at column (k % per_row) S, row (k / per_row) S.  Texel (x, y) of a
 *              block belongs to the even face iff x + y <= S - 1, else to the odd one.  Corner texels: even (1, 1), (S - 4, 1), (1, S - 4); odd (S - 2, S - 2),
 *              (3, S - 2), (S - 2, 3).  The hypotenuses x + y = S - 3 and x + y = S + 1 keep a bilinear fetch inside either triangle on its owner's texels.
 *   unweld     vertices' [3 f + k] = vertex k of face f, faces' [f] = (3 f, 3 f + 1, 3 f + 2), uv at the corner texel (col, row) of the atlas:
 *              u = (double)col / Wt, v = 1.0 - (double)row / Ht (hive_render_shade's nearest-texel rule lands on that texel).
 *   fill       texel (x, y) of a block, owner f: even b1 = (x - 1) / (S - 5), b2 = (y - 1) / (S - 5); odd b1 = (S - 2 - x) / (S - 5), b2 = (S - 2 - y) / (S - 5);
 *              b0 = (1 - b1) - b2 (the gutter extrapolates the same map).  With a view: P_r = (b0 V0_r + b1 V1_r) + b2 V2_r; cam and c in hive_project's order
 *              (above, "vertex") with the view's R, t; when !(c_2 >= near) -- only a gutter point can be -- P is replaced by V0, which the draw kept.  Sample
 *              point u = min(max(c_0 / c_2, 0), W - 1), v = min(max(c_1 / c_2, 0), H - 1) (pixel centres at integers; this clamps the four taps to the image);
 *              j0 = floor(u), i0 = floor(v), j1 = min(j0 + 1, W - 1), i1 = min(i0 + 1, H - 1), ax = u - j0, ay = v - i0; per channel
 *              top = c00 + ax (c01 - c00), bottom = c10 + ax (c11 - c10), c = top + ay (bottom - top); texel = (uint8)min(255, max(0, floor(c + 0.5))).
 *              Without a view: c = (b0 a0 + b1 a1) + b2 a2 of the three vertex colours, the same rounding.  Texels whose owner is >= nf are 0.
 * All pointers named d_ are device memory; K is a host array.  Nothing synchronises. */
/* One view's vote.  d_faces i32 [nf][3] with ids in [0, nv) (a face with another id is skipped), d_xy i32 [nv][2] and d_z f64 [nv] of that view's hive_render_draw,
 * d_depth f32 [H][W] of its hive_render_resolve, d_mask u8 [H][W] (may be NULL: nothing masked; non-zero = do not use), 0 <= view_index < 65535,
 * depth_tolerance >= 0, d_best u64 [nf] in / out (zeroed by the caller before the first view). */
int hive_texture_select(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, const int32_t *d_xy, const double *d_z, const float *d_depth,
                        const uint8_t *d_mask, int H, int W, int view_index, double depth_tolerance, uint64_t *d_best);
/* The atlas of nf faces (host arithmetic, no launch, no context): *Wt, *Ht, *per_row (each may be NULL).  HIVE_ERR_INVALID: nf outside [1, 2^31), cell outside
 * [6, 64], a side above 16384. */
int hive_texture_layout(int64_t nf, int cell, int *Wt, int *Ht, int *per_row);
/* d_vertices f64 [nv][3], d_faces i32 [nf][3] -> d_vertices_out f64 [3 nf][3], d_faces_out i32 [nf][3], d_uv f64 [3 nf][2]; with d_views i32 [nf] (may be NULL)
 * also the winning view of d_best u64 [nf] (may be NULL), 65535 - (key & 65535), or -1 for none.  3 nf < 2^31. */
int hive_texture_unweld(hive_ctx *ctx, const double *d_vertices, int64_t nv, const int32_t *d_faces, int64_t nf, int cell, const uint64_t *d_best,
                        double *d_vertices_out, int32_t *d_faces_out, double *d_uv, int32_t *d_views);
/* The atlas d_texture u8 [Ht][Wt][3] of hive_texture_layout(nf, cell): the welded mesh (d_vertices, d_vertex_colors u8 [nv][3], d_faces), d_best of the selects,
 * the n <= 65535 frames d_frames u8 [n][H][W][3], K and d_poses f64 [n][12] = per view R row-major then t (world-to-camera).  A key naming a view >= n counts as
 * no view.  near > 0. */
int hive_texture_fill(hive_ctx *ctx, const double *d_vertices, int64_t nv, const uint8_t *d_vertex_colors, const int32_t *d_faces, int64_t nf, const uint64_t *d_best,
                      const uint8_t *d_frames, int n, int H, int W, const double K[9], const double *d_poses, double near, int cell, uint8_t *d_texture);

/* ---- smoothing the view labels across edges -- csrc/texture_smooth.hip.  hive_texture_select lets every face decide alone; where two views see a surface about
 * equally well neighbouring faces flip between them, and every flip is a seam.  The three entry points below keep the areas in a table, build the edge
 * adjacency of the mesh and move labels while that lowers E = -sum_f area[L[f]][f] + seam_cost * #seams.  Integers only; the result is the same whatever order
 * workgroups run in and however many rounds the host issues between two polls.  This is iterated conditional modes: it ends in a LOCAL optimum of E, it is not
 * a graph cut.  Out of scope: a chart atlas (unweld and fill are unchanged: 3 F vertices, cell^2 texels per face pair), blending; exposure gains and seam levelling are
 * further down (hive_texture_samples).  The rules:
 *   vote        hive_texture_select's candidate test, on the same d_xy, d_z, d_depth and d_mask, and a filter on the sign of the snapped area A: facing 0 takes
 *               either sign (as select does), 1 only A < 0, -1 only A > 0.  d_area[view_index nf + f] = |A| of a candidate, 0 otherwise; every entry of the row is
 *               written.  Which sign is the front: measured on the marching-cubes mesh of the tests' fused room (2 052 faces, three views) under the
 *               rasteriser's snap, 7 / 9 / 31 candidates have A > 0 (seen from behind) and 881 / 1 090 / 1 163 have A < 0: for this project's meshes
 *               front-facing means A < 0, so facing = 1 is the back-face test hive_texture_select lacks.
 *   neighbours  face g is an edge-neighbour of f (g != f) once for every unordered pair of vertex ids that is an edge of both: two faces sharing two edges list
 *               each other twice, duplicates of a face three times, an edge with m faces gives each of them m - 1 entries.  A face with an id outside [0, nv)
 *               or a repeated id has no entries and appears in none.  d_offsets[f] .. d_offsets[f + 1] are f's entries in d_neighbours, ascending.  Cost: per face
 *               edge (a, b) a walk over the faces of a, and an insertion sort of the face's entries -- quadratic in a face's degree, fine for surfaces.
 *   smooth      start: L[f] = the view v with the largest d_area[v][f] > 0, on equal area the lower v, -1 if there is none.  One round, read entirely from the
 *               labels at its start: for every f with L[f] = cur >= 0, cnt(x) = the number of f's neighbour entries g with L[g] = x; for each label l != cur that
 *               some neighbour entry holds, with d_area[l][f] != 0, gain(l) = (area[l][f] - area[cur][f]) + seam_cost (cnt(l) - cnt(cur)); f PROPOSES the l of
 *               largest gain, on a tie the lower l, if that gain is > 0; f APPLIES its proposal iff for every neighbour entry g that proposes, gain_f > gain_g,
 *               or the gains are equal and mix32(f) < mix32(g) (mix32: x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16 on 32 bits,
 *               the decimation's bijection; with the plain index a tied 32 x 32 grid needs 32 rounds instead of 4).  An unlabelled neighbour counts for
 *               nothing, and an unlabelled face stays so.  Appliers are pairwise non-adjacent, so a round lowers E by exactly the sum of their gains (a seam = a
 *               neighbour entry (f, g), f < g, with both labels >= 0 and different; the adjacency is symmetric); E is a bounded integer, so the rounds end.
 *               They stop at the first round without a proposal; `rounds` counts the rounds before it.  More than 4096: HIVE_ERR_STATE.
 *               end: d_best[f] = 0 if L[f] < 0, else area[L[f]][f] << 16 | (65535 - L[f]): hive_texture_select's key format, which unweld and fill take as it is.
 *               With seam_cost = 0 nothing can propose (a tie has gain 0), so with facing = 0 the keys are those n calls of hive_texture_select leave.
 *               Magnitudes: areas < 2^47, seam_cost < 2^40, a face's degree < 2^16 (refused otherwise): gains stay below 2^47 + 2^56.
 * Memory: the table is 8 n_views nf bytes (186 MB for 725 k faces and 32 views). */
/* One view's row of the table: the arguments of hive_texture_select, facing in {-1, 0, 1}, d_area i64 [n_views][nf].  (view_index + 1) nf < 2^31, else
 * HIVE_ERR_INVALID: a table has n_views nf < 2^31 entries. */
int hive_texture_vote(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, const int32_t *d_xy, const double *d_z, const float *d_depth,
                      const uint8_t *d_mask, int H, int W, int view_index, double depth_tolerance, int facing, int64_t *d_area);
/* The edge adjacency of d_faces i32 [nf][3] (3 nf < 2^31) over nv vertices: d_offsets i64 [nf + 1], d_neighbours i32 [capacity] (may be NULL with capacity 0),
 * *total = the number of entries.  One read-back; when capacity < *total the call fails with HIVE_ERR_INVALID and the total in its message, *total is set
 * and nothing is written to d_neighbours: call again with that capacity.  A closed manifold has 3 nf entries. */
int hive_mesh_face_neighbours(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, int64_t *d_offsets, int32_t *d_neighbours, int64_t capacity,
                              int64_t *total);
/* The labelling.  d_area i64 [n_views][nf] with entries in [0, 2^47), 1 <= n_views <= 65535, n_views nf < 2^31; d_offsets i64 [nf + 1] and d_neighbours i32
 * [n_entries] as hive_mesh_face_neighbours writes them (checked on the device: offsets ascending from 0 to at most n_entries, ids in [0, nf), no face its own
 * neighbour, a degree below 2^16; HIVE_ERR_INVALID otherwise); 0 <= seam_cost < 2^40 in the table's unit; rounds_per_poll: the rounds issued between two
 * read-backs of the device's state, 0 = the default of 8 (the result does not depend on it).  d_best u64 [nf] out; stats (may be NULL) = {rounds, label
 * changes, seam entries before, seam entries after, area given up = sum_f (max_v area[v][f] - area[L[f]][f])}.  Synchronises once per batch of rounds. */
int hive_texture_smooth(hive_ctx *ctx, const int64_t *d_area, int n_views, int64_t nf, const int64_t *d_offsets, const int32_t *d_neighbours, int64_t n_entries,
                        int64_t seam_cost, int rounds_per_poll, uint64_t *d_best, int64_t stats[5]);

/* ---- exposure gains and seam levelling -- csrc/texture_level.hip.  The labels above decide WHERE the texture changes from one key frame to another; key frames
 * of a camera with auto-exposure or auto white balance disagree in brightness and tint, and every remaining label change then shows as a step.  Two corrections,
 * both off unless asked for: one multiplicative gain per key frame and channel (samples, sums, a host solve), and additive offsets that close the step at every
 * seam vertex and fade out harmonically inside each patch (level).  hive_texture_fill_adjusted applies both.  Restated in
 * tests/texture_levelling_restatement.py.  Out of scope: a border between a textured and an untextured face is not levelled; blending of several views; a chart
 * atlas.  The rules (float64, no fused multiply-add, in the order written; a sum written "in order" starts at 0.0 and adds term after term):
 *   samples     once per view, right after that view's hive_texture_vote, on the same d_xy.  A face with d_area[view][f] != 0 takes its three vertices' nearest
 *               pixels ((Y_k + 128) >> 8, (X_k + 128) >> 8), the ones the vote tested.  If all nine bytes lie in [1, 254] the sample is the per-channel sum of
 *               the three pixels (3 .. 762); otherwise, and for every other face, it is (0, 0, 0) = invalid (a clipped pixel says nothing about gain).
 *               d_samples u16 [n_views][nf][3]; every entry of the row is written.  6 n_views nf bytes.
 *   sums        a face is valid in a view iff its three sums there are non-zero.  Over the faces valid in both a and b, a != b:
 *               G[c][a][b] = sum s_af s_bf, D[c][a][b] = sum s_af^2 (a's energy inside its overlap with b), N[a][b] = their number; diagonals 0.  Integers
 *               below 2^51: the order of addition does not matter.  n_views <= 256.
 *   solve       (the host's, numpy float64, per channel; hive_amd.texturing.solve_gains) e_a = sum_b D[a][b] exactly; M_aa = (double)e_a + prior (double)e_a,
 *               M_ab = -(double)G[a][b], rhs_a = prior (double)e_a; a view with e_a = 0: the identity row, rhs 1.  g = solve(M, rhs) -- Brown and Lowe's gain
 *               compensation with the prior weighted by the data's own energy, so `prior` has no unit.  The prior shrinks every gain, so over the views with
 *               e_a > 0, summed in ascending a: g <- g (sum e_a) / (sum e_a g_a).  q = clip(floor(g 65536 + 0.5), 16384, 262144), u32 Q16.  A channel whose
 *               solve fails or gives a gain that is not finite or not positive keeps q = 65536 for every view.  The device sees only q.
 *   level       a face PARTICIPATES iff it has a view (key != 0, view < n), its ids lie in [0, nv) and are distinct; label l = its view.  Every other face has
 *               offsets 0 and is invisible to the rule.  A NODE is a pair (vertex v, label l) that some participating face has.  Its colour c(v, l), per
 *               channel: fill's sample at P = V_v with view l (the same projection, clamp and bilinear, unrounded; no near test: the view's draw kept the
 *               vertex), then (c (double)q[l][ch]) 2^-16.  A SEAM VERTEX has two or more distinct labels among its participating faces; there
 *               m(v) = (the sum in order of c(v, l) over its labels ascending) / count, and node (v, l) is FIXED at h = m(v) - c(v, l).  Every other node
 *               starts at 0.  Then `sweeps` Jacobi sweeps, each read entirely from the buffer before it: a node (v, l) that is not fixed becomes
 *               (the sum in order, over the participating faces f with label l that hold v, ascending f, v at corner k, of h[f][(k + 1) % 3] then
 *               h[f][(k + 2) % 3]) / (2 count), h[f][j] being the offset of node (faces[f][j], l).  d_offsets f64 [nf][3][3] = per face corner and channel the
 *               offset of its node.  The vertex -> faces lists are sorted by insertion: quadratic in a vertex's degree, fine for surfaces.
 *   adjusted fill  hive_texture_fill's rule; with a view: texel = byte(((c (double)q[view][ch]) 2^-16) + ((b0 h0 + b1 h1) + b2 h2)), h_k = d_offsets[f][k][ch]
 *               (the gutter extrapolates the same affine map); without a view the vertex colours, as the plain fill.  With every q = 65536 and every h = 0
 *               both extra operations are exact and the atlas is hive_texture_fill's bit for bit. */
/* One view's row of d_samples u16 [n_views][nf][3]: d_faces, d_xy of that view's hive_render_draw, d_area i64 [n_views][nf] with that view's row written by
 * hive_texture_vote, d_frame u8 [H][W][3] that view's frame.  (view_index + 1) nf < 2^31. */
int hive_texture_samples(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, const int32_t *d_xy, const int64_t *d_area, const uint8_t *d_frame, int H,
                         int W, int view_index, uint16_t *d_samples);
/* The pair sums of a finished table into HOST arrays G i64 [3][n_views][n_views], D i64 [3][n_views][n_views], N i64 [n_views][n_views].  1 <= n_views <= 256
 * (HIVE_ERR_INVALID above), n_views nf < 2^31.  Workgroups reduce before they add: one 64-bit atomic per workgroup, pair and word.  One read-back. */
int hive_texture_exposure_sums(hive_ctx *ctx, const uint16_t *d_samples, int n_views, int64_t nf, int64_t *G, int64_t *D, int64_t *N);
/* The offsets d_offsets f64 [nf][3][3] of `level`: the welded mesh, the final keys d_best, the frames, K and d_poses as hive_texture_fill takes them,
 * d_gains_q16 u32 [n][3] (all 65536: no gains), 0 <= sweeps <= 4096 (one launch each; nothing waits).  3 nf < 2^31.  *seam_vertices and *max_offset (the
 * largest |offset|; each may be NULL) cost one read-back. */
int hive_texture_level(hive_ctx *ctx, const double *d_vertices, int64_t nv, const int32_t *d_faces, int64_t nf, const uint64_t *d_best, const uint8_t *d_frames, int n,
                       int H, int W, const double K[9], const double *d_poses, const uint32_t *d_gains_q16, int sweeps, double *d_offsets, int64_t *seam_vertices,
                       double *max_offset);
/* hive_texture_fill with gains and offsets (neither NULL): see `adjusted fill`. */
int hive_texture_fill_adjusted(hive_ctx *ctx, const double *d_vertices, int64_t nv, const uint8_t *d_vertex_colors, const int32_t *d_faces, int64_t nf,
                               const uint64_t *d_best, const uint8_t *d_frames, int n, int H, int W, const double K[9], const double *d_poses, double near, int cell,
                               const uint32_t *d_gains_q16, const double *d_offsets, uint8_t *d_texture);

/* ---- ray casting the volume and tracking the camera against it (KinectFusion-style frame-to-model ICP; no counterpart in the reference, which takes its
 * poses from COLMAP or BundleFusion).  Float32 where stated, every operation rounded once (no fused multiply-add), in the order written here; pixel (u, v) =
 * (column, row), pixel centres at integers.
 *   ray        d = ((u - cx) / fx, (v - cy) / fy, 1); R, t = cam_pose (camera-to-world) rounded to float32 once; w_r = (R[r][0] d_0 + R[r][1] d_1) + R[r][2].
 *              The ray parameter is camera z: P_r(z) = z w_r + t_r, and in voxel coordinates p_r(z) = (P_r(z) - origin_r) / voxel_size.
 *   range      z_in = z_near, z_out = z_far (+inf for z_far <= 0); per axis r, with g0 = (t_r - origin_r) / voxel_size, gd = w_r / voxel_size and
 *              hi = dim_r - 1 (the box of voxel centres): gd != 0: a = (0 - g0) / gd, b = (hi - g0) / gd, z_in = max(z_in, min(a, b)), z_out = min(z_out,
 *              max(a, b)); gd == 0: no hit unless 0 <= g0 <= hi.  No hit unless z_in <= z_out.
 *   sample     S(p): valid iff 0 <= p_r < dim_r - 1 on every axis and the eight corners floor(p) + {0, 1}^3 have weight > 0.  With f = p - floor(p) and T the
 *              tsdf plane: c_xy = T[x][y][z0] + f_z (T[x][y][z1] - T[x][y][z0]); c_x = c_x0 + f_y (c_x1 - c_x0); S = c_0 + f_x (c_1 - c_0).
 *   march      step = step_in_trunc * trunc; z_k = z_in + (float)k step for k = 0 .. min(floor((z_out - z_in) / step), 2^20).  The first k with S(z_{k-1})
 *              valid and > 0 and S(z_k) valid and <= 0 is the hit: z* = z_{k-1} + (step S_{k-1}) / (S_{k-1} - S_k).  A valid pair going < 0 to > 0 (leaving a
 *              surface from behind) ends the ray without a hit.  An invalid sample never pairs with a valid one.
 *   outputs    depth = z* (0 without a hit: the convention of depth maps and of hive_render_resolve's depth plane); vertex = P(z*), world frame; normal =
 *              g / sqrt((g_x g_x + g_y g_y) + g_z g_z) with g_r = S(p* + e_r) - S(p* - e_r), p* = p(z*): unit length, pointing into free space; (0, 0, 0) if
 *              one of the six samples is invalid or the length is 0 (depth and vertex are still written); colour = the packed colour of voxel
 *              clamp(floor(p* + 0.5), 0, dim - 1), unpacked r, g, b.  A pixel without a hit is all zeros in every plane.
 * d_depth f32 [H][W], d_vertex f32 [H][W][3], d_normal f32 [H][W][3], d_color u8 [H][W][3]: device memory, any may be NULL.  K f32 3 x 3 and cam_pose f64 4 x 4
 * are host arrays.  z_near >= 0; step_in_trunc > 0 (0.5 in the Python wrapper).  An x-slab volume is refused with HIVE_ERR_INVALID.  Nothing synchronises. */
int hive_tsdf_raycast(hive_tsdf *vol, int H, int W, const float K[9], const double cam_pose[16], float z_near, float z_far, float step_in_trunc, float *d_depth,
                      float *d_vertex, float *d_normal, uint8_t *d_color);
/* The depth pyramid of a live frame with its vertex and normal maps (camera frame, float32).  d_depth f32 [H][W] metres, 0 = invalid (a sample counts when it
 * is > 0).  Level 0 is the frame; level l + 1 has size (floor(H_l / 2), floor(W_l / 2)) and its pixel (u, v) comes from the samples (2v, 2u), (2v, 2u + 1),
 * (2v + 1, 2u), (2v + 1, 2u + 1) of level l: m = the smallest valid one; sum and count, in that order, of the valid ones with d - m <= pyr_delta; the result
 * is sum / count, or 0 for a block without a valid sample.  Level intrinsics: fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2 carried in float64 from level
 * to level and rounded to float32 per level (level 0: K as given); K_levels (host, f32 [levels][9]) receives them.
 *   vertex     V = ((d (u - cx)) / fx, (d (v - cy)) / fy, d); (0, 0, 0) where d is not valid
 *   normal     a = V(u + 1, v) - V, b = V(u, v + 1) - V; c = a x b = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x); N = c / sqrt((c_x c_x + c_y c_y) +
 *              c_z c_z), negated when (N_x V_x + N_y V_y) + N_z V_z > 0, so that it faces the camera like the ray cast's normals face free space.  (0, 0, 0)
 *              on the last row and column, where one of the three depths is not valid, or where the length is 0 or not finite.
 * The levels are packed back to back: d_depth_pyr f32 [sum H_l W_l], d_vertex_pyr and d_normal_pyr f32 [sum H_l W_l][3].  1 <= levels <= 8 and the last
 * level must not be empty.  Nothing synchronises. */
int hive_frame_maps(hive_ctx *ctx, const float *d_depth, int H, int W, const float K[9], int levels, float pyr_delta, float *d_depth_pyr, float *d_vertex_pyr,
                    float *d_normal_pyr, float *K_levels);
/* One Gauss-Newton step's sums of frame-to-model point-to-plane ICP at one pyramid level.  d_live_vertex / d_live_normal: the live frame's maps (camera frame,
 * hive_frame_maps); d_model_vertex / d_model_normal: the volume ray cast at model_pose with this level's size and K (world frame, hive_tsdf_raycast).  A map
 * pixel is valid iff its normal is not (0, 0, 0).  Per valid live pixel, in float64 from the float32 maps, with R, t = est_pose and M = model_pose^-1 =
 * [R_m^T | -((R_m^T[r][0] t_0 + R_m^T[r][1] t_1) + R_m^T[r][2] t_2)] (both camera-to-world, host f64 4 x 4):
 *   q_r = ((R[r][0] V_0 + R[r][1] V_1) + R[r][2] V_2) + t_r;  n_r = (R[r][0] N_0 + R[r][1] N_1) + R[r][2] N_2;  c = M q in q's order
 *   kept iff c_z > 0; (pu, pv) = round(fx (c_x / c_z) + cx), round(fy (c_y / c_z) + cy) with the context's rounding mode lies inside the image; the model maps
 *   are valid there; with d = V_m - q: sqrt((d_0 d_0 + d_1 d_1) + d_2 d_2) <= dist_thresh; (n_0 N_m0 + n_1 N_m1) + n_2 N_m2 >= cos_thresh
 *   r = (N_m0 d_0 + N_m1 d_1) + N_m2 d_2;  J = [q x N_m, N_m] = (q_1 N_m2 - q_2 N_m1, q_2 N_m0 - q_0 N_m2, q_0 N_m1 - q_1 N_m0, N_m0, N_m1, N_m2)
 * h_sums (host, 28): J_i J_j for i <= j row by row (21), J_i r (6), r r.  Minimising sum (r - J xi)^2 over xi = (omega, v) is A xi = b with A, b from these
 * sums; the update is T <- [exp(omega) | v] T.  The sums are added in a fixed order -- pixel e = v W + u belongs to workgroup e / 256, thread e % 256; per
 * workgroup the tree x[t] += x[t + off] for off = 128, 64 .. 1; then the workgroups' results in ascending order from 0.0 -- so every run gives the same bits
 * (no floating-point atomic).  h_pairs (host): the number of kept pairs; without any, the sums are zeros.  d_pair_mask u8 [H][W] (device, may be NULL): 1
 * where the live pixel was kept.  Synchronises the stream (one copy of 29 numbers). */
int hive_icp_step(hive_ctx *ctx, int H, int W, const float K[9], const float *d_live_vertex, const float *d_live_normal, const float *d_model_vertex,
                  const float *d_model_normal, const double model_pose[16], const double est_pose[16], float dist_thresh, float cos_thresh, double *h_sums,
                  int64_t *h_pairs, uint8_t *d_pair_mask);
/* The intensity pyramid of a live colour frame, for the photometric term below.  d_color u8 [H][W][3] (r, g, b).  Level 0 is Y / 255 in float32 with the
 * integer luma Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 (hive_jpeg_encode's); level l + 1 has hive_frame_maps' sizes (floor(H_l / 2), floor(W_l / 2))
 * and its pixel (u, v) is ((a + b) + (c + d)) * 0.25f over the samples (2v, 2u), (2v, 2u + 1), (2v + 1, 2u), (2v + 1, 2u + 1) of level l.  The levels are
 * packed back to back: d_gray_pyr f32 [sum H_l W_l].  1 <= levels <= 8 and the last level must not be empty.  Nothing synchronises. */
int hive_gray_pyramid(hive_ctx *ctx, const uint8_t *d_color, int H, int W, int levels, float *d_gray_pyr);
/* hive_icp_step with the photometric term of RGB-D odometry (Steinbruecker et al. 2011, Kerl et al. 2013; Open3D's "hybrid" odometry) beside it, in one pass
 * and with one copy back.  h_sums (host, 56) and h_pairs (host, 2): the first 28 sums and the first count are hive_icp_step's for the same inputs, bit for
 * bit; the second 28 and the second count are the photometric term's.  Further inputs: d_live_gray f32 [H][W], this level of hive_gray_pyramid; d_model_depth
 * f32 [H][W] and d_model_color u8 [H][W][3], the depth and colour planes of the ray cast that gave d_model_vertex.  The model's intensity I at a pixel is
 * Y / 255 (float32) of its colour, as above.  Per live pixel with V_z > 0 (its normal is not needed), in float64 from the float32 maps:
 *   project    q and c = M q as in hive_icp_step; kept iff c_z > 0; pu = fx (c_x / c_z) + cx, pv = fy (c_y / c_z) + cy, not rounded
 *   cell       x0 = floor(pu), y0 = floor(pv); kept iff 1 <= x0 <= W - 3 and 1 <= y0 <= H - 3 (so a picture with H < 4 or W < 4 has no photometric pairs);
 *              a = pu - x0, b = pv - y0
 *   gradients  at an integer model pixel gx = 0.5 (I(x + 1, y) - I(x - 1, y)), gy = 0.5 (I(x, y + 1) - I(x, y - 1)); the pixel is usable iff its ray-cast depth
 *              and that of its four neighbours are > 0; kept iff the cell's corners (x0 + {0, 1}, y0 + {0, 1}) are all usable
 *   sampling   for each of I, gx, gy with A_ji its value at (x0 + i, y0 + j): top = A00 + a (A01 - A00), bot = A10 + a (A11 - A10), value = top + b (bot - top)
 *   occlusion  xn = x0 + (a >= 0.5), yn = y0 + (b >= 0.5); kept iff |D_m(yn, xn) - c_z| <= dist_thresh
 *   r = I_live(u, v) - I;  g_c = ((gx fx) / c_z, (gy fy) / c_z, -(((gx fx) c_x + (gy fy) c_y) / (c_z c_z)));  g_w = R_m g_c, row r in the order
 *   (R_m[r][0] g_c0 + R_m[r][1] g_c1) + R_m[r][2] g_c2 (R_m the rotation of model_pose);  J = [q x g_w, g_w], written out like hive_icp_step's J
 * -J is the derivative of r by xi, as for the geometric term, so the two sets of normal equations add: A = A_geo + w^2 A_photo, b = b_geo + w^2 b_photo with
 * w in metres per unit of intensity (the caller's; hive_amd.tracking.icp_align).  The 21 + 6 + 1 sums and the count are added in hive_icp_step's order.
 * d_photo_mask u8 [H][W] (device, may be NULL): 1 where the live pixel was kept for this term.  Synchronises the stream (one copy of 58 numbers). */
int hive_rgbd_icp_step(hive_ctx *ctx, int H, int W, const float K[9], const float *d_live_vertex, const float *d_live_normal, const float *d_live_gray,
                       const float *d_model_vertex, const float *d_model_normal, const float *d_model_depth, const uint8_t *d_model_color,
                       const double model_pose[16], const double est_pose[16], float dist_thresh, float cos_thresh, double *h_sums, int64_t *h_pairs,
                       uint8_t *d_pair_mask, uint8_t *d_photo_mask);

/* ---- scoring a render against a held-out frame -- compare_images(ref_image, est_image), scripts/compare_image_pair.py:110-133, and ms_ssim as called at
 * scripts/experiments.py:1627-1635; the loops that use them are experiments.py:775-858 (LLFF) and :1554-1637 (HyperNeRF).  Pictures are u8 [N][H][W][3] in
 * device memory and stay there.  Three libraries are restated from their published definitions; none of them can be run beside this code, so the numbers are
 * not pinned against cv2 (gray), not pinned against skimage (SSIM, PSNR) and not pinned against pytorch_msssim (MS-SSIM).  tests/similarity_restatement.py states
 * the same rules in numpy / torch-CPU float64.  The rules (no fused multiply-add anywhere):
 *   gray       cv2's 8-bit COLOR_BGR2GRAY of OpenCV 3.4, from recall: g = (1868 c0 + 9617 c1 + 4899 c2 + 8192) >> 14, c0 c1 c2 the channels in memory order,
 *              all integer, result u8.  The reference hands RGB pictures to this BGR conversion, so channel 0 gets the blue weight: that is what its numbers
 *              contain and it is the default (rgb_order = 0).  rgb_order = 1 swaps the two outer weights (true luma of an RGB picture).
 *   mask       variant 1 (`variants` = 2) is masked_frame[color_np == [255, 255, 255]] = 255 of experiments.py:846-848 / :1605-1607.  The comparison
 *              broadcasts, so the rule is per CHANNEL, not per pixel: a channel value of the reference picture reads as 255 wherever the estimate's value in
 *              that same channel is 255.  Applied while loading; the whitened frame is never written.  Variant 0 is the plain pair.
 *   SSIM       skimage.metrics.structural_similarity(ref_gray, est_gray, win_size=7) on u8: data_range 255, K1 0.01, K2 0.03, uniform 7 x 7 window, sample
 *              covariance, float64; the score is the mean of the map cropped by 3 pixels a side, so every window lies inside the picture and no border rule
 *              exists.  The five window sums Sx, Sy, Sxx, Syy, Sxy (x = ref gray, y = est gray; at most 49 * 255^2) are exact int32.  Then in float64, in
 *              exactly this order:
 *                ux = Sx / 49.0, uy, uxx, uyy, uxy likewise;  vx = (49.0 / 48.0) * (uxx - ux * ux), vy likewise;  vxy = (49.0 / 48.0) * (uxy - ux * uy);
 *                C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
 *                S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)),   sums evaluated left to right.
 *              The map S [H - 6][W - 6] is reproducible bit for bit in numpy.
 *   SSIM sum   a workgroup owns a 32 x 32 tile of the map (row-major, p = 32 r + c).  Thread t of 256 adds its valid S(p) for p = t, t + 256, t + 512, t + 768 in
 *              that order to 0.0; then v[t] += v[t + off] for t < off, off = 128, 64, ..., 1; v[0] is the tile's partial.  hive_similarity_finish sums the
 *              partials of one picture: thread t adds partials t, t + 256, ... in ascending order to 0.0, the same tree follows, and the sum is divided by the
 *              divisor.  No floating-point atomic exists, so a score has the same bits on every run and in whatever batch the picture came.
 *   PSNR       skimage.metrics.peak_signal_noise_ratio on the two gray planes: the device returns the exact integer sum of squared differences over all H W
 *              pixels (one 64-bit integer atomic per workgroup); the caller computes 10 * log10(65025.0 / (sse / (H * W))) in float64, inf when sse == 0.
 *   MS-SSIM    pytorch_msssim.ms_ssim(X, Y, data_range=1.0, size_average=True): the three colour channels as float64 c / 255.0 (the mask rule applies to X);
 *              window g[11] given by the caller (a Gaussian, sigma 1.5: exp(-(i - 5)^2 / (2 sigma^2)) over its sum), applied separably, first along H then
 *              along W, no padding, each a sum of g[k] * value over ascending k.  Per level and channel with C1 = 0.01 * 0.01, C2 = 0.03 * 0.03:
 *                mu1 = G(X), mu2 = G(Y);  s1 = G(X X) - mu1 mu1, s2 = G(Y Y) - mu2 mu2, s12 = G(X Y) - mu1 mu2;
 *                cs = (2 s12 + C2) / (s1 + s2 + C2);  ssim = ((2 mu1 mu2 + C1) / (mu1 mu1 + mu2 mu2 + C1)) * cs.
 *              Five levels, weights 0.0448 0.2856 0.3001 0.2363 0.1333; levels 0-3 contribute relu(mean(cs)), level 4 relu(mean(ssim)); between levels both
 *              pictures pass a 2 x 2 average pool of stride 2, padded by size % 2 at the low end of each axis, the padding zeros counted (every window is
 *              divided by 4, avg_pool2d's count_include_pad=True).  The score is the mean over the channels of the product of value ^ weight.  The smaller
 *              side must exceed 160 (the original asserts).  Sums over a map: a workgroup owns 16 x 32 values (p = 32 r + c, thread t adds p = t, t + 256) and
 *              reduces as above; hive_similarity_finish then gives the mean.
 * LPIPS is restated below, above hive_lpips_create; MIFD (SIFT keypoints, the exact matcher) below that, above hive_sift_create.  Nothing synchronises; every call is ordered on the context's stream. */
/* compare_images' SSIM and PSNR sums (compare_image_pair.py:120-124) for N pairs and `variants` (1: plain; 2: plain, then masked) at once.  H, W >= 7, N >= 1,
 * variants * N <= 65535.  d_partials f64 [variants][N][ceil((H - 6) / 32) * ceil((W - 6) / 32)]: the tile sums of S, for hive_similarity_finish with the divisor
 * (H - 6)(W - 6).  d_sse i64 [variants][N]: zeroed here, then the sum of squared gray differences.  Optional (NULL = not stored): d_map f64 [variants][N][H - 6][W - 6],
 * d_gray_ref u8 [variants][N][H][W], d_gray_est u8 [N][H][W]. */
int hive_similarity_ssim_psnr(hive_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_est, int N, int H, int W, int rgb_order, int variants, double *d_partials,
                              int64_t *d_sse, double *d_map, uint8_t *d_gray_ref, uint8_t *d_gray_est);
/* One level of ms_ssim (experiments.py:1630-1635).  Input, exactly one of: the pictures d_ref_u8 / d_est_u8 u8 [N][h][w][3] (level 0), or the planes d_x f64
 * [variants][N][3][h][w] and d_y f64 [N][3][h][w] a previous level left.  h, w >= 11.  window: host f64 [11].  d_partials f64 [2][variants * N * 3][T] with
 * T = ceil((h - 10) / 16) * ceil((w - 10) / 32): tile sums of the cs map, then of the ssim map, rows in (variant, picture, channel) order, for
 * hive_similarity_finish with the divisor (h - 10)(w - 10).  d_x_next f64 [variants][N][3][h2][w2] and d_y_next f64 [N][3][h2][w2], h2 = (h + 1) / 2, w2 = (w + 1) / 2:
 * the pooled planes of the next level (both NULL after the last level).  variants * N * 3 <= 65535. */
int hive_similarity_msssim_level(hive_ctx *ctx, const uint8_t *d_ref_u8, const uint8_t *d_est_u8, const double *d_x, const double *d_y, int N, int h, int w,
                                 int variants, const double window[11], double *d_partials, double *d_x_next, double *d_y_next);
/* d_out[r] = (the sum of d_partials[r][0 .. per_row), in the fixed order above) / divisor, for r < rows: a picture's score does not depend on the batch. */
int hive_similarity_finish(hive_ctx *ctx, const double *d_partials, int64_t rows, int64_t per_row, double divisor, double *d_out);
/* The product over the levels: d_means f64 [5][2][count][3] (level; cs mean, ssim mean; variant * N + picture; channel) as hive_similarity_finish left them ->
 * d_out f64 [count] = mean over the channels of prod_l max(value_l, 0) ^ weight_l, value_l the cs mean for l < 4 and the ssim mean for l = 4. */
int hive_similarity_msssim_combine(hive_ctx *ctx, const double *d_means, int64_t count, double *d_out);

/* ---- LPIPS: the third score of a render -- lpips.LPIPS(net='alex') as scripts/compare_image_pair.py:29-41 feeds it and :110-133 returns it; the loops and tables
 * that use it are scripts/experiments.py:663-684, :844-852 (plain and masked), :1384-1426 and scripts/compare_image_pairs.py:40-84.  The lpips package and
 * torchvision are absent, so the network is restated from its published definition (lpips 0.1, eval mode, version 0.1 linear layers over torchvision's AlexNet
 * features) and the numbers are not pinned against lpips / torchvision.  tests/lpips_restatement.py states the same rules in torch-CPU and numpy.  The rules (no
 * fused multiply-add outside the MFMA's own chain):
 *   input      u8 [N][H][W][3]; channel k of the picture is channel k of the network (no reordering: the reference hands LPIPS whatever order its pictures are
 *              in).  The value of a byte v is ((v / 255) * 2.0 - 1.0) in float64, rounded to float32 (compare_image_pair.py:30-33); the scaling layer then
 *              gives (x - shift[k]) / scale[k] in float32, shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  The host builds this 3 x 256 float32
 *              table once with exactly these operations and the kernel looks values up.
 *   mask       variant 1 (`variants` = 2) is experiments.py:846-848 as for hive_similarity_ssim_psnr: per CHANNEL, a reference byte reads as 255 where the
 *              estimate's byte of the same pixel and channel is 255; applied while loading, the whitened frame is never written.
 *   features   the five ReLU maps, float32 [pictures][h][w][C] (channels last), each a convolution with bias, then ReLU:
 *                0: conv 3 -> 64, 11 x 11, stride 4, pad 2;   1: maxpool 3 / 2, conv 64 -> 192, 5 x 5, pad 2;   2: maxpool 3 / 2, conv 192 -> 384, 3 x 3, pad 1;
 *                3: conv 384 -> 256, 3 x 3, pad 1;   4: conv 256 -> 256, 3 x 3, pad 1.   The maxpool is floor mode without padding: (h - 3) / 2 + 1.
 *              Inputs, weights, accumulation and outputs are float32.  A value is the chain acc = fma(x_k, w_k, acc) from 0.0f over k = (ky, kx, ci) ascending
 *              (__builtin_amdgcn_mfma_f32_32x32x2f32; padding and the tail of K add fma(0, 0, acc)), then acc + bias, then max with 0.  Its bits depend on the
 *              receptive field and the weights alone: not on the picture's place in the batch, on N, or on the slot (reference / estimate).  There is no
 *              split-K and no floating-point atomic.  Against exact arithmetic |error| <= gamma_K (sum |w| |x| + |b|), gamma_K = K u / (1 - K u), u = 2^-24, K the
 *              layer's products plus the bias: 364, 1601, 1729, 3457, 2305.
 *   tail       not pinned against lpips: the package does this in float32; here, per layer and pixel, from the float32 vectors a (reference) and b (estimate) of
 *              C channels, in float64, every sum over c ascending, added left to right to 0.0:
 *                na = sqrt(sum a_c a_c) + 1e-10, nb likewise;   t_c = a_c / na - b_c / nb;   d = sum w_c * (t_c * t_c),   w the layer's 1 x 1 linear weights.
 *   sums       a workgroup owns 256 consecutive pixels p of one picture's map (thread t holds d(p), 0.0 past the end), the tree v[t] += v[t + off], off = 128 ..
 *              1, gives its partial; hive_similarity_finish adds a picture's partials and divides by h w: the layer's score.  The LPIPS of a pair is
 *              l0 + l1 + l2 + l3 + l4, added left to right.  The same bits on every run and in every batch.
 * Nothing synchronises; every call is ordered on the context's stream (the workspace grows, with a synchronisation, when a call needs more than any before). */
typedef struct hive_lpips hive_lpips;
/* lpips.LPIPS(net='alex') from host float32 weights in torch's shapes: conv_w[l] OIHW [C_out][C_in][k][k], conv_b[l] [C_out], lin_w[l] [C_out] (the 1 x 1 linear
 * layer lin{l}.model.1.weight, [1][C][1][1]) for the five rows above.  Repacks the weights on the device and builds the input table. */
int hive_lpips_create(hive_ctx *ctx, const float *const conv_w[5], const float *const conv_b[5], const float *const lin_w[5], hive_lpips **out);
/* Frees the model and its workspace (after the stream has drained). */
int hive_lpips_destroy(hive_lpips *net);
/* One row of the feature table of the network compare_image_pair.py:29-41 runs: d_in f32 [N][h][w][C_in], the previous row's ReLU map, un-pooled (layer 0: the scaled picture, [N][H][W][3]) -> d_out f32
 * [N][ho][wo][C_out].  Both 16-byte aligned.  hive_lpips_forward runs the same launchers. */
int hive_lpips_layer(hive_lpips *net, int layer, const float *d_in, int N, int h, int w, float *d_out);
/* The LPIPS of N pairs (compare_image_pair.py:29-41; experiments.py:844-848 with variants = 2: plain, then masked).  H, W >= 31: the smallest picture with an
 * output in every layer (7, 3, 1, 1, 1).  d_scores f64 [variants][N].  Optional (NULL = not stored): d_layer_scores f64 [5][variants][N]; d_features[l] f32
 * [variants + 1][N][h_l][w_l][C_l], the features of the reference, of the masked reference when asked, then of the estimate (computed once for both variants);
 * d_dist[l] f64 [variants][N][h_l][w_l], the maps d.  Any N: the pairs are run in chunks over one workspace. */
int hive_lpips_forward(hive_lpips *net, const uint8_t *d_ref_u8, const uint8_t *d_est_u8, int N, int H, int W, int variants, double *d_scores,
                       double *d_layer_scores, float *const d_features[5], double *const d_dist[5]);

/* ---- SIFT, the exact matcher and MIFD: the fourth score of a render -- mifd() of scripts/compare_image_pair.py:44-97 (cv2.SIFT.create(), a 2-nearest-neighbour
 * descriptor match, Lowe's ratio test, the mean distance between matched keypoint positions); the detector is also what hive/pose_optimisation.py:294, :426, :452
 * call.  cv2 is absent: the rules below are Lowe's SIFT with the parameters and rules of cv2.SIFT.create() as recalled from OpenCV 4.x, and the result is not
 * pinned against cv2.  The reference matches with FLANN, an approximate randomised KD-tree search; the matcher here is the exact answer and is not pinned against
 * FLANN.  tests/sift_restatement.py states the same rules in numpy float32.  All arithmetic is float32 with one rounding per operation (no fused multiply-add),
 * sqrt and / correctly rounded, sums evaluated left to right; rint is round-half-even.
 *   exp        E(x), x clamped to >= -87: n = rint(x * f(1.4426950408889634)); r = x - n * 0.693145751953125; r = r - n * f(1.42860682030941723212e-6);
 *              p = f(1/5040); p = p r + f(1/720); p = p r + f(1/120); p = p r + f(1/24); p = p r + f(1/6); p = p r + 0.5; p = p r + 1; p = p r + 1;
 *              E = ldexp(p, n).  f(.) rounds a float64 constant to float32.  Relative error below 2^-21 for -87 <= x <= 10.
 *   atan2      A(y, x) in degrees (cv2's fastAtan2 form): ax = |x|, ay = |y|, e = f(2.220446049250313e-16), p1 = f(0.9997878412794807 * 57.29577951308232),
 *              p3 = f(-0.3258083974640975 * 57.29577951308232), p5 = f(0.1555786518463281 * 57.29577951308232), p7 = f(-0.04432655554792128 * 57.29577951308232);
 *              if ax >= ay: c = ay / (ax + e), a = (((p7 c^2 + p5) c^2 + p3) c^2 + p1) c; else c = ax / (ay + e), a = 90 - (that polynomial);
 *              x < 0: a = 180 - a; y < 0: a = 360 - a.  Within 0.3 degrees of atan2 (cv2's stated accuracy; the polynomial's own error is near 0.01).
 *   sin, cos   of a degrees in [0, 360]: q = rint(a * f(1/90)); t = (a - q * 90) * f(pi / 180); u = t t;
 *              s = ((((f(1/362880) u + f(-1/5040)) u + f(1/120)) u + f(-1/6)) u + 1) t;  c = ((((f(-1/3628800) u + f(1/40320)) u + f(-1/720)) u + f(1/24)) u - 0.5) u + 1;
 *              (cos, sin) = (c, s), (-s, c), (-c, -s), (s, -c) for q mod 4 = 0, 1, 2, 3.
 *   base       gray u8 -> float32; x2 bilinear with INTER_LINEAR's geometry, source coordinate (d + 0.5) / 2 - 0.5, edge samples replicated (the weights are 0.25
 *              and 0.75: exact); then a blur by sqrt(max(sigma^2 - 4 * 0.5^2, 0.01)).  The first octave is -1.
 *   octaves    round(log2(min(2H, 2W)) - 2) + 1 of them, each nOctaveLayers + 3 layers; layer i is layer i - 1 blurred by sig[i] = sqrt((sigma k^i)^2 -
 *              (sigma k^(i-1))^2), k = 2^(1 / nOctaveLayers); the next octave's layer 0 is layer nOctaveLayers at every second row and column, (rows / 2, cols / 2)
 *              rounded down.
 *   blur       separable, border reflect-101 folded as often as the radius needs (a 3 x 4 octave meets 25 taps); round(8 sig + 1) | 1 taps, exp(-(i - R)^2 /
 *              (2 sig^2)) in float64 over their sum, rounded to float32, GIVEN BY THE CALLER (as the MS-SSIM window is) so that one set of bits serves the device
 *              and a restatement; at most 33.  Along the row first, then along the column: out = t[0] v[0], then + t[k] v[k] for k = 1 .. ascending.
 *   extrema    DoG i = layer i + 1 - layer i.  threshold = floor(0.5 * contrastThreshold / nOctaveLayers * 255) (contrastThreshold as float32); border 5; a
 *              candidate of DoG 1 .. nOctaveLayers has |v| > threshold and is >= all 26 neighbours (v > 0) or <= all of them (v < 0).
 *   refine     up to 5 steps: with s = f(1/255), first derivatives (difference) * (s * 0.5), second (sum - 2 v) * s, mixed (a - b - c + d) * (s * 0.25) in cv2's
 *              operand order; solve H X = dD by elimination on the 3 x 4 matrix with partial pivoting (largest |a| in the column, lowest row on a tie; a zero
 *              pivot rejects), back substitution X2 = a23 / a22, X1 = (a13 - a12 X2) / a11, X0 = (a03 - a01 X1 - a02 X2) / a00; offset = -X.  All |offset| < 0.5
 *              ends the loop; an offset that is not <= 2^29 in magnitude rejects; else c, r, layer move by rint(offset) and leaving layers 1 .. nOctaveLayers or
 *              the border rejects; five steps without the end reject.  contr = v s + (dD . offset) * 0.5 (the dot as d0 xc + d1 xr + d2 xi); reject on |contr| *
 *              nOctaveLayers < contrastThreshold, on det = dxx dyy - dxy dxy <= 0, on tr^2 edge >= (edge + 1)(edge + 1) det.  Then x = (c + xc) 2^o, y likewise,
 *              octave = o + (layer << 8) + (rint((xi + 0.5) * 255) << 16), size = sigma * E(((layer + xi) / nOctaveLayers) * f(ln 2)) * 2^o * 2, response = |contr|.
 *   mask       a candidate is dropped when mask[(int)(y * 0.5 + 0.5)][(int)(x * 0.5 + 0.5)] (clamped into the picture) is 0: before orientation.
 *   nfeatures  > 0: before orientation a candidate stays when fewer than nfeatures candidates of its picture have a larger response (the nfeatures largest and
 *              everything equal to the last of them).
 *   orient     scl = size * 0.5 / 2^o; radius rint(4.5 scl); weight E((i^2 + j^2) * (-1 / (2 (1.5 scl)^2))); samples p = (i + radius)(2 radius + 1) + (j + radius)
 *              of the window whose pixel lies strictly inside the layer: dx = right - left, dy = up - down, bin = rint(f(0.1) * A(dy, dx)) mod 36, value weight *
 *              sqrt(dx dx + dy dy).  Lane p mod 64 adds its samples in ascending p to a private histogram; bin totals are 0 + lane 0 + lane 1 + ... + lane 63.
 *              Smoothed h[b] = (t[b-2] + t[b+2]) / 16 + (t[b-1] + t[b+1]) * 0.25 + t[b] * 0.375.  Every b with h[b] > both neighbours and >= 0.8 max h gives a
 *              keypoint: bin = b + 0.5 (h[l] - h[r]) / (h[l] - 2 h[b] + h[r]) wrapped into [0, 36), angle = 360 - 10 bin, 0 when within FLT_EPSILON of 360.
 *   keypoint   (x * 0.5, y * 0.5, size * 0.5, angle, response, octave) with the octave byte (o - 1) & 255: six float32 (the packed octave is below 2^24).  Sorted by
 *              that tuple, exact duplicates removed.
 *   descriptor 4 x 4 x 8, on the keypoint's layer at its octave: point rint(x 2^-octave), rint(y 2^-octave); ori = 360 - angle (0 when within FLT_EPSILON of 360);
 *              hist_width = 3 (size 2^-octave 0.5); radius = min(rint(hist_width * f(sqrt 2) * 5 * 0.5), (int)sqrt(rows^2 + cols^2)); cos and sin of ori divided by
 *              hist_width; per window sample p as above: c_rot = j cos - i sin, r_rot = j sin + i cos, rbin = r_rot + 2 - 0.5, cbin likewise, kept when both lie
 *              in (-1, 4) and the pixel strictly inside; weight E((c_rot^2 + r_rot^2) * (-1 / 8)); obin = (A(dy, dx) - ori) * f(8 / 360); trilinear split in cv2's
 *              order (v_r1 = mag rbin, v_r0 = mag - v_r1, ...) into the eight bins (r0 + 0/1, c0 + 0/1, o0 / o0 + 1 mod 8), in the order 000 001 010 011 100 101 110
 *              111; rows and columns outside 0 .. 3 take nothing.  Lane-private histograms and the lane-order sum as for the orientation.  Then nrm2 = sum of
 *              squares ascending; clip at sqrt(nrm2) * 0.2; nrm2 again; scale 512 / max(sqrt(nrm2), FLT_EPSILON); rint, saturated to 0 .. 255, stored as bytes.
 *   knn        squared L2 distance of byte descriptors: an exact integer (at most 128 * 255^2 < 2^24); the two nearest, a tie to the lower train index; distance
 *              = float32 sqrt of the integer; index -1 and +inf where the train set has fewer than two.
 *   MIFD       a query q survives when d0 < ratio * d1 in float32; its residual is (x_q - x_t, y_q - y_t) in float32, its length sqrt(dx dx + dy dy) in float64;
 *              the score is the float64 sum over the survivors in query order divided by their number; nan with fewer than 2 descriptors on either side or fewer
 *              than min_matches (or no) survivors.
 * Every stage has the same bits on every run, in every batch and at every place in it: no floating-point atomic exists; the appends are integer atomics and the
 * sort removes their order.  Nothing synchronises; every call is ordered on the context's stream.  A picture with more candidates or keypoints than `capacity` is
 * never cut silently: d_counts holds the true counts, and the caller fails the call when one exceeds the capacity (hive_amd.features does, naming the count). */
typedef struct hive_sift hive_sift;
/* A detector for pictures of H x W (>= 6 x 6), up to max_images (<= 8192) a call, `capacity` (<= 65535) candidates and keypoints a picture.  nOctaveLayers 1 .. 5.
 * taps[i] / tap_counts[i], i = 0 .. nOctaveLayers + 2: host float32 blur taps, [0] the base blur, [i] the blur from layer i - 1 to layer i (rule `blur`). */
int hive_sift_create(hive_ctx *ctx, int H, int W, int max_images, int nfeatures, int n_octave_layers, double contrast_threshold, double edge_threshold, double sigma,
                     const float *const *taps, const int *tap_counts, int capacity, hive_sift **out);
/* Frees the detector (after the stream has drained). */
int hive_sift_destroy(hive_sift *sift);
/* d_gray u8 [N][H][W]; d_mask u8 [N][H][W] or NULL -> d_keypoints f32 [N][capacity][6], d_descriptors u8 [N][capacity][128] (4-byte aligned), d_counts i32 [N][3]:
 * refined candidates, keypoints before the duplicates left, keypoints.  Rows past a count are undefined.  1 <= N <= max_images. */
int hive_sift_detect(hive_sift *sift, const uint8_t *d_gray, const uint8_t *d_mask, int N, float *d_keypoints, uint8_t *d_descriptors, int32_t *d_counts);
/* Stages of the most recent hive_sift_detect, for the tests: a Gaussian layer f32 [N][rows][cols] of an octave (octave 0 is 2H x 2W, each next one halved, rounded
 * down); the refined candidates [N][capacity][8] 32-bit words in append order: x, y, size, response (f32, before the halving), packed octave, layer, r, c (i32). */
int hive_sift_read_layer(hive_sift *sift, int octave, int layer, int N, float *d_out);
int hive_sift_read_candidates(hive_sift *sift, int N, void *d_out);
/* For tools/probe_sift.py, which times the stages by difference: hive_sift_detect stops after the pyramid (stage 1: the counts stay 0) or after the sorted
 * keypoints (stage 2: no descriptors); 0, the default, runs everything. */
int hive_sift_set_last_stage(hive_sift *sift, int stage);
/* The two nearest of T train descriptors for each of Q query descriptors (u8 [.][128], 4-byte aligned): d_indices i32 [Q][2], d_distances f32 [Q][2] (rule `knn`). */
int hive_knn_match(hive_ctx *ctx, const uint8_t *d_query, int Q, const uint8_t *d_train, int T, int32_t *d_indices, float *d_distances);
/* MIFD of `pairs` pairs from hive_sift_detect's outputs over pictures [.][capacity]: pair p matches picture query_first + p against picture train_first + p.
 * d_indices i32 and d_distances f32 [pairs][capacity][2] receive the matches, d_scores f64 [pairs] the score, d_matches i32 [pairs] the survivors. */
int hive_mifd(hive_ctx *ctx, const float *d_keypoints, const uint8_t *d_descriptors, const int32_t *d_counts, int capacity, int query_first, int train_first, int pairs,
              float ratio_threshold, int min_matches, int32_t *d_indices, float *d_distances, double *d_scores, int32_t *d_matches);

/* ---- Feature pairs for pose optimisation: FeatureExtractor of hive/pose_optimisation.py:437-578 behind hive_sift_detect -- the 2-nearest-neighbour match of an
 * arbitrary list of picture pairs, the ratio-and-depth filter (:518-539), a homography RANSAC where the reference calls cv2.findHomography(..., cv2.USAC_MAGSAC)
 * (:562) and the compaction by its inlier mask.  cv2 is absent and USAC_MAGSAC is randomised: the RANSAC below is an exact rule of its own and is not pinned
 * against cv2 (as the keypoints are not pinned against cv2's SIFT and the matcher is not pinned against FLANN).  tests/ransac_restatement.py states the same
 * rules in numpy.  The RANSAC's arithmetic is float64 with one rounding per operation (no fused multiply-add), sqrt and / correctly rounded; parentheses below
 * give the order.
 *   match      rule `knn` above between picture pairs[p][0] (queries) and picture pairs[p][1] (trains).
 *   filter     a pair whose pictures do not both have max(min_features, 2) keypoints has no rows.  Query q survives when NOT (double) d0 > ratio * (double) d1
 *              (the float32 distances widened, the product in float64: the reference's Python arithmetic, not MIFD's float32 <), and depth_i[r(y_q)][r(x_q)] != 0
 *              and depth_j[r(y_t)][r(x_t)] != 0, r(v) = rint(v) on the float32 coordinate (half-even) clamped into the picture.  Survivors keep the order of q:
 *              a row is x_q, y_q, x_t, y_t, depth_i, depth_j (float32), q, t (int32).  Counts per pair: ratio survivors, survivors.
 *   M < 4      M correspondences (x, y) -> (u, v) a pair, float32 widened.  M < 4: no model (mask 0, H NaN, winning trial -1, counts 0).  A count outside
 *              0 .. stride is refused, never cut: no model, winning trial -2.
 *   lane sum   L(v) over items k = 0 .. M - 1: lane l = 0 .. 63 adds v[l], v[l + 64], ... in ascending order to 0.0; L = 0.0 + lane 0 + lane 1 + ... + lane 63.
 *   normalise  per side: cx = L(x) / M, cy = L(y) / M, m = L(sqrt((x - cx)(x - cx) + (y - cy)(y - cy))) / M, s = 1.4142135623730951 / m; NOT m > 0 on either
 *              side: no model.  X = (x - cx_i) s_i, Y = (y - cy_i) s_i, U = (u - cx_j) s_j, V = (v - cy_j) s_j.
 *   draw       mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (lowbias32, uint32).  base = mix(mix(mix(seed) ^ frame_i) ^
 *              frame_j), the pair key (frame_i, frame_j) from the caller (the frames, not the place in the batch); h = mix(base ^ t) for trial t; draw k = 0 .. 3:
 *              r_k = mulhi(mix(h ^ k), M - k), taken as the r_k-th index not yet chosen, in ascending order.  The sample keeps the order drawn.
 *   solve      sample point k gives rows 2k: [X, Y, 1, 0, 0, 0, -(U X), -(U Y) | U] and 2k + 1: [0, 0, 0, X, Y, 1, -(V X), -(V Y) | V] (h33 = 1).  Elimination on
 *              the 8 x 9 matrix, column c = 0 .. 7: pivot = the largest |a[r][c]|, r >= c, the lowest row on a tie; |pivot| <= eps = 2^-40 rejects the trial
 *              (a degenerate sample; normalised coordinates are of order 1); rows exchanged; for r > c: f = a[r][c] / a[c][c], a[r][k] = a[r][k] - f a[c][k] for
 *              k > c.  Back substitution r = 7 .. 0: acc = a[r][8]; acc = acc - a[r][k] h[k] for k = r + 1 .. 7 ascending; h[r] = acc / a[r][r].
 *   score      w = (h6 X + h7 Y) + 1; pu = (h0 X + h1 Y) + h2; pv = (h3 X + h4 Y) + h5; du = pu / w - U; dv = pv / w - V; e2 = du du + dv dv; an inlier has
 *              w > 0 and e2 <= thr thr, thr = threshold s_j: `threshold` target pixels, the target normalisation being a similarity.  The score is the integer
 *              count.  All `trials` trials run (no early stop).  The winner has the largest count, the lower t on a tie: one 64-bit integer atomic maximum a pair
 *              of count << 32 | (0xFFFFFFFF - t).  All trials rejected: no model.
 *   refit      once, over the winner's inliers: G[a][b] (a <= b) and g[a] are lane sums over the inliers (a lane's items ascending; per item first
 *              + r1[a] r1[b], then + r2[a] r2[b]; g with the right-hand sides), r1 and r2 the two rows above; G mirrored, the same elimination.  Re-scored; the
 *              refit's h and mask are kept when it solved and counts at least the winner's, else the winner's.
 *   H          A = h T_i: A[r][0] = h[r][0] s_i, A[r][1] = h[r][1] s_i, A[r][2] = (h[r][2] - A[r][0] cx_i) - A[r][1] cy_i; B = T_j^-1 A: B[0][c] = A[0][c] / s_j +
 *              cx_j A[2][c], B[1][c] = A[1][c] / s_j + cy_j A[2][c], B[2][c] = A[2][c]; H = B / B[2][2].
 *   compact    a pair is kept when it has min_features survivors and min_features inliers (:457-468); the kept pairs' inlier rows follow each other in pair order,
 *              inliers in row order.
 * No floating-point atomic; the same bits on every run, in every batch and at every place in it.  Nothing synchronises. */
/* hive_sift_detect's outputs over N pictures [.][capacity], d_pairs i32 [P][2] picture indices (a pair naming a picture outside 0 .. N - 1 has no rows),
 * d_depth f32 [N][H][W] -> d_rows [P][capacity][8] 32-bit words (16-byte aligned; rows past a pair's count are undefined), d_pair_counts i32 [P][2].  Optional
 * (both or neither): the raw table d_indices i32 and d_distances f32 [P][capacity][2].  1 <= P <= 65535. */
int hive_pairs_match(hive_ctx *ctx, const float *d_keypoints, const uint8_t *d_descriptors, const int32_t *d_counts, int capacity, int N, const int32_t *d_pairs, int P,
                     const float *d_depth, int H, int W, double ratio, int min_features, float *d_rows, int32_t *d_pair_counts, int32_t *d_indices, float *d_distances);
/* P pairs of correspondences: pair p has d_counts[p * count_stride] rows of row_words 32-bit words (the first four: x, y, u, v float32) from d_rows + p * stride *
 * row_words on; d_keys i32 [P][2] the pair keys -> d_H f64 [P][9], d_mask u8 [P][stride] (0 past the count), d_result i32 [P][3]: the winning trial (-1: no
 * model, -2: count outside 0 .. stride), the winner's count, the final count.  A pair with fewer than max(min_count, 4) correspondences has no model (:457-460). */
int hive_ransac_homography(hive_ctx *ctx, const float *d_rows, int row_words, const int32_t *d_counts, int count_stride, const int32_t *d_keys, int P, int stride,
                           double threshold, int trials, unsigned seed, int min_count, double *d_H, uint8_t *d_mask, int32_t *d_result);
/* hive_pairs_match's rows and counts, hive_ransac_homography's mask and result -> d_out [.][8] (room for P * stride rows, 16-byte aligned), d_kept i32 [P] the rows
 * of every pair (0: dropped), d_offsets i64 [P + 1] the rows before every pair and, last, all rows. */
int hive_pairs_compact(hive_ctx *ctx, const float *d_rows, const int32_t *d_pair_counts, const uint8_t *d_mask, const int32_t *d_result, int P, int stride,
                       int min_features, float *d_out, int32_t *d_kept, int64_t *d_offsets);

/* ---- frame registration from 3-D feature matches: a rigid (optionally similarity) RANSAC on the back-projected rows of hive_pairs_match -- csrc/register.hip.
 * It stands where the reference shells out to COLMAP (estimate_pose) and names BundleFusion; cv2's estimateAffine3D, Open3D's correspondence RANSAC, BundleFusion
 * and COLMAP are all absent, so the rules below are this project's own and are pinned against none of them.  tests/rigid_restatement.py states the same rules in
 * numpy.  Float64 with one rounding per operation (no fused multiply-add), sqrt and / correctly rounded; parentheses give the order; `lane sum` and `draw` are
 * the rules above hive_pairs_match.
 *   points     with a camera (fx, fy, cx, cy) a row is x_i, y_i, x_j, y_j, depth_i, depth_j (float32, widened): Z = depth, X = ((x - cx) Z) / fx,
 *              Y = ((y - cy) Z) / fy on either side; p the point of side i, q of side j.  Without a camera (NULL) the first six words of a row are
 *              X_i Y_i Z_i X_j Y_j Z_j.  M < max(min_count, 3): no model.  A count outside 0 .. stride is refused, never cut (winning trial -2).
 *   draw       the first three draws (k = 0, 1, 2) of rule `draw`: three distinct indices below M, in the order drawn.
 *   degenerate per side e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), a . b = (ax bx + ay by) + az bz:
 *              the sample is rejected when n . n <= (2^-20 (e1 . e1)) (e2 . e2) on either side (sin^2 of the angle at p0 at most 2^-20: scale-free; two equal
 *              points give 0 <= 0).
 *   horn       one solver for the minimal sample and the refit.  Centroids cp, cq; p' = p - cp, q' = q - cq; S[a][b] = sum p'_a q'_b, sp = sum p' . p',
 *              sq = sum q' . q'.  Minimal sample: cp = ((p0 + p1) + p2) / 3 per component, the sums over k = 0, 1, 2 in the order drawn, each added to 0.0.
 *              N (symmetric 4 x 4): N00 = (Sxx + Syy) + Szz, N11 = (Sxx - Syy) - Szz, N22 = (Syy - Sxx) - Szz, N33 = (Szz - Sxx) - Syy, N01 = Syz - Szy,
 *              N02 = Szx - Sxz, N03 = Sxy - Syx, N12 = Sxy + Syx, N13 = Szx + Sxz, N23 = Syz + Szy.  Cyclic Jacobi, V = I, S_w = 7 sweeps (measured: 5 reach
 *              an off-diagonal norm of 2^-52 of the Frobenius norm on every committed case; two more) over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a
 *              rotation is skipped when a_pq is exactly 0; theta = (a_qq - a_pp) / (2 a_pq); t = sign(theta) / (|theta| + sqrt(theta theta + 1)),
 *              sign(theta) = 1 for theta >= 0; c = 1 / sqrt(t t + 1); s = t c; a_pp = a_pp - t a_pq, a_qq = a_qq + t a_pq, a_pq = 0; for the two other r:
 *              a_rp = c a_rp - s a_rq and a_rq = s a_rp + c a_rq (both from the old values); for r = 0 .. 3 the same with V[r][p], V[r][q].
 *              (w, x, y, z) = the column of V at the largest a_kk, the lowest k on a tie; negated when w < 0, or when w == 0 and the first non-zero of x, y, z
 *              is negative; divided by n = sqrt(((w w + x x) + y y) + z z).  R00 = ((w w + x x) - y y) - z z, R01 = 2 (x y - w z), R02 = 2 (x z + w y),
 *              R10 = 2 (x y + w z), R11 = ((w w - x x) + y y) - z z, R12 = 2 (y z - w x), R20 = 2 (x z - w y), R21 = 2 (y z + w x),
 *              R22 = ((w w - x x) - y y) + z z.  scale = sqrt(sq / sp) with with_scale, else 1; A = scale R per entry; t_r = cq_r - ((A_r0 cp_x + A_r1 cp_y) +
 *              A_r2 cp_z).  No model when sp or sq is 0 or sp, sq, scale or an entry of A or t is not finite.
 *   inlier     d_r = (((A_r0 p_x + A_r1 p_y) + A_r2 p_z) + t_r) - q_r; an inlier has d . d <= threshold threshold, `threshold` in the depth's unit (a NaN is not
 *              an inlier).  The score is the integer count.  All `trials` trials run (no early stop).  The winner has the largest count, the lower trial on
 *              a tie: one 64-bit integer atomic maximum a pair of count << 32 | (0xFFFFFFFF - trial).  All trials rejected: no model.
 *   refit      once, by `horn` over the winner's n inliers in two passes of lane sums: cp = L(p) / n, cq = L(q) / n; then S, sp, sq as lane sums of the centred
 *              terms.  Re-scored; the refit's model and mask are kept when it solved and counts at least the winner's, else the winner's.
 *   outputs    T = [A | t; 0 0 0 1] maps camera-i points onto camera-j points; scale; rms = sqrt(L(d . d over the final inliers) / final count).  Without a
 *              model T, scale and rms are NaN and the mask is 0.
 * No floating-point atomic; the same bits on every run, in every batch and at every place in it.  Nothing synchronises. */
/* P pairs of correspondences as for hive_ransac_homography, row_words >= 6; `camera`: four doubles fx, fy, cx, cy on the HOST, read during the call, or NULL for
 * the points layout -> d_T f64 [P][16], d_scale f64 [P], d_rms f64 [P], d_mask u8 [P][stride] (0 past the count), d_result i32 [P][3]: the winning trial (-1: no
 * model, -2: count outside 0 .. stride), the winner's count, the final count. */
int hive_ransac_rigid(hive_ctx *ctx, const float *d_rows, int row_words, const int32_t *d_counts, int count_stride, const int32_t *d_keys, int P, int stride,
                      const double *camera, double threshold, int trials, unsigned seed, int min_count, int with_scale, double *d_T, double *d_scale, double *d_rms,
                      uint8_t *d_mask, int32_t *d_result);

/* ---- glTF 2.0 export: the meshes of a scene packed into the binary buffer of a .glb -- what Pipeline._write_mesh_to_disk (hive/pipeline.py:921-936) hands to
 * trimesh's exporter and Pipeline._compress_with_draco (:938-980) to draco_transcoder -- csrc/gltf.hip.  trimesh, pygltflib and draco_transcoder are absent: the
 * bytes below are stated from the glTF 2.0 specification and KHR_mesh_quantization and are not pinned against trimesh's exporter or against three.js's loader.
 * tests/gltf_restatement.py states the same rules in numpy.  Float64 arithmetic with one rounding per operation, / correctly rounded, rint = round half to even.
 *   views      one binary buffer; mesh after mesh, within a mesh POSITION, TEXCOORD_0 (with uv), COLOR_0 (with colours), indices.  Every view starts at the next
 *              multiple of 4 after the view before it, the bytes between are 0, and the buffer ends on a multiple of 4.
 *   bounds     per mesh and axis lo = min, hi = max over the vertices (float32 input widened).  A vertex that is not finite fails the call.
 *   quantize 0 POSITION 3 x float32: the round-to-nearest-even cast of the input.  TEXCOORD_0 2 x float32 of (u, 1.0 - v), the subtraction in float64 (the atlas
 *              coordinates of pack_textures_row have their origin bottom-left, glTF's top-left).  COLOR_0 4 x uint8 normalised: r, g, b (each through lut[.] when
 *              a table is given), a (255 when the input has three channels; never through the table).  Indices uint32.
 *   quantize 1 KHR_mesh_quantization.  s = (hi - lo) / 65535.0 per axis, s = 1.0 when hi == lo.  POSITION 3 x uint16, not normalised, in an 8-byte stride whose
 *              last two bytes are 0: q = min(65535, rint((x - lo) / s)); the mesh's node carries scale s and translation lo.  TEXCOORD_0 2 x uint16 normalised:
 *              rint(min(max(c, 0.0), 1.0) * 65535.0) of c = u and c = 1.0 - v.  COLOR_0 as above.  Indices uint16 when V <= 65535, else uint32.
 *   indices    an index outside [0, V) fails the call.  A mesh without faces (or without vertices) is rejected: leave its node out.
 * Failures name the first mesh they concern.  No floating-point atomic; the same bytes on every run, for a mesh alone or inside a batch. */
typedef enum hive_gltf_kind { HIVE_GLTF_POSITION = 0, HIVE_GLTF_TEXCOORD = 1, HIVE_GLTF_COLOR = 2, HIVE_GLTF_INDICES = 3 } hive_gltf_kind;
typedef enum hive_gltf_dtype { HIVE_GLTF_F32 = 0, HIVE_GLTF_F64 = 1, HIVE_GLTF_I32 = 0, HIVE_GLTF_I64 = 1 } hive_gltf_dtype;
typedef struct hive_gltf_mesh {
    const void *vertices;   /* device [V][3], vertex_dtype */
    const void *faces;      /* device [F][3], face_dtype */
    const double *uv;       /* device [V][2] or NULL */
    const uint8_t *colors;  /* device [V][color_channels] or NULL */
    int64_t n_vertices, n_faces;
    int32_t vertex_dtype;   /* HIVE_GLTF_F32 / HIVE_GLTF_F64 */
    int32_t face_dtype;     /* HIVE_GLTF_I32 / HIVE_GLTF_I64 */
    int32_t color_channels; /* 3 or 4 (read only with colours) */
    int32_t reserved;
} hive_gltf_mesh;
typedef struct hive_gltf_view {
    int64_t offset, length; /* bytes; an absent view is {0, 0} */
} hive_gltf_view;
/* Host only (no context, no device; the pointers of a mesh are only tested against NULL) -> views[n][4] indexed by hive_gltf_kind, *total_bytes the buffer's
 * length.  A failure's message is hive_last_error(NULL). */
int hive_gltf_layout(const hive_gltf_mesh *meshes, int n, int quantize, hive_gltf_view *views, int64_t *total_bytes);
/* Three launches for any n (bounds, bounds final stage, pack) behind ONE upload of the descriptor table: d_out (device, 4-byte aligned, out_bytes >= the layout's
 * total) receives every view and the padding inside the layout's total; bounds (host) [n][2][3] = lo, hi per mesh in float64.  lut: 256 bytes in host memory or
 * NULL.  Returns after the device has finished (the bounds come back with the error words). */
int hive_gltf_pack(hive_ctx *ctx, const hive_gltf_mesh *meshes, int n, int quantize, const uint8_t *lut, uint8_t *d_out, int64_t out_bytes, double *bounds);

/* ---- baseline JPEG: the textures of a glTF file (`image/jpeg`) encoded on the device -- csrc/jpeg.hip.  The reference embeds PNG (trimesh) and has no such
 * step.  The bytes are libjpeg's, as Pillow (libjpeg-turbo) writes them with quality = q, subsampling 4:4:4 or 4:2:0, optimize = False, restart_marker_rows = 1;
 * tests/jpeg_restatement.py states the same rules in numpy and tests/test_jpeg_cpu.py pins that restatement against Pillow, whole files.  Integer arithmetic only.
 *   tables     Annex K quantisation tables scaled by 5000 / q (q < 50) or 200 - 2 q: clip((base * scale + 50) / 100, 1, 255); the four Annex K Huffman tables.
 *   colour     Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;
 *              Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 *   edges      the MCU is 8 x 8 (4:4:4) or 16 x 16 (4:2:0).  Columns past the width repeat the last column at full resolution.  Rows past the height repeat
 *              the last row, except the chroma of 4:2:0: there rows repeat up to an EVEN height, the picture is down-sampled, and the last DOWN-SAMPLED row
 *              repeats.  Down-sampling: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, .. along the output row.
 *   transform  samples - 128, libjpeg's slow integer DCT (Loeffler, Ligtenberg, Moschytz; CONST_BITS 13, PASS1_BITS 2; rows, then columns), quantised as
 *              sign(c) * ((|c| + (d >> 1)) / d), d = table << 3.
 *   dummies    luminance blocks of 4:2:0 past ceil(W / 8) or ceil(H / 8): zero AC; past the right edge the DC of the block to the left in the MCU, in a
 *              row past the bottom the DC of Y01 in both blocks.
 *   scan       one interleaved scan (Y00 Y01 Y10 Y11 Cb Cr, or Y Cb Cr), zigzag order, DC differences per component, run / size codes with ZRL and EOB,
 *              0x00 behind every 0xFF.  The restart interval is one MCU row: 1-bits up to the byte, RST(n mod 8), predictors back to 0; EOI behind the last.
 *   header     SOI, APP0 (JFIF 1.1, density 1 x 1, no units), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, DRI, SOS: 629 bytes.
 * The same bytes on every run, for a picture alone or anywhere in a batch. */
typedef enum hive_jpeg_subsampling { HIVE_JPEG_444 = 0, HIVE_JPEG_420 = 2 } hive_jpeg_subsampling; /* Pillow's numbers */
typedef struct hive_jpeg_image {
    const uint8_t *data; /* device [height][pitch] bytes: width pixels of R, G, B at the start of every row */
    int32_t height, width;
    int64_t pitch;       /* bytes from one row to the next, >= 3 * width */
} hive_jpeg_image;
/* Host only (no context, no device) -> offsets[n], each a multiple of 4, and *total_bytes: room for the WORST case of every file.  A block's longest coding is
 * a DC code of 11 bits with 11 value bits and 63 AC coefficients of a 16-bit code with 10 value bits each (a ZRL or EOB only replaces longer codes):
 * 22 + 63 * 26 = 1660 bits, taken as 52 words = 208 bytes.  Stuffing can at most double every byte: 416 bytes per block.  Every MCU row adds a marker of 2
 * bytes (its padding to a byte is inside the block bound), the file 629 bytes of header: bound = 629 + 416 * blocks + 2 * MCU rows, up to a multiple of 4,
 * blocks = MCUs * 3 (4:4:4) or * 6 (4:2:0).  Fails on n < 1, an unknown subsampling, a side of 0 or above 65535; the message is hive_last_error(NULL). */
int hive_jpeg_layout(const hive_jpeg_image *images, int n, int subsampling, int64_t *offsets, int64_t *total_bytes);
/* Seven launches for any n behind ONE upload of the picture table: file i goes to d_out + offsets[i] (device; out_bytes >= the layout's total, or the call fails
 * naming the bytes needed, before any launch; nothing is ever written past out_bytes), its length to sizes[i] (host).  quality 1 .. 100.  At most 2^22 blocks
 * per call.  Returns after the device has finished (the sizes come back in one small copy). */
int hive_jpeg_encode(hive_ctx *ctx, const hive_jpeg_image *images, int n, int quality, int subsampling, uint8_t *d_out, int64_t out_bytes, int64_t *sizes);

/* ---- PNG: depth maps, masks and textures encoded on the device -- csrc/png.hip.  Lossless: the decoded pixels are the input's; the bytes are this encoder's own
 * (not zlib's, not Pillow's) and a function of the picture's bytes alone: the same on every run, for a picture alone or anywhere in a batch.
 * tests/png_restatement.py states the same rules in numpy.  Integer arithmetic only.
 *   file       signature, IHDR (no interlace), ONE IDAT, IEND.  Gray 8 / gray 16 (colour type 0; 16-bit samples most significant byte first) / RGB 8 (type 2).
 *   IDAT       one zlib stream: 78 01, the deflate blocks, the Adler-32 of the filtered rows.  Chunk CRC-32s and the Adler-32 are combined on the device from
 *              per-segment parts by the bytes that follow each part; nothing walks the bytes serially.
 *   filter     per row all five filters against the RAW row above (zeros above the first); the smallest sum of |signed byte| wins, ties to the lowest type.
 *              Stated, and not pinned against Pillow's filter heuristic (equal on smooth pictures, not on noisy ones).
 *   segments   the filtered stream (a filter byte in front of every row) is cut every S = 8192 bytes; a segment becomes ONE dynamic block (BTYPE 2), or one
 *              stored block where the dynamic coding below is not smaller than 5 + its bytes.  Noise never expands beyond the stored form.
 *   joining    byte-aligned: behind every dynamic block but the last an EMPTY stored block (000, zeros up to the byte, 00 00 FF FF).  The last block carries
 *              BFINAL and is padded with zeros.
 *   matches    at position p (room = min(258, bytes to the end of p's segment)) three candidate distances: the bytes of one pixel; one row (row bytes + 1);
 *              p minus the nearest earlier position whose three bytes equal p's three (exact equality, from a stable sort of the positions by those bytes; p's
 *              three bytes must lie inside the picture).  A candidate counts if 1 <= distance <= min(p, 32768); its length is the run of equal bytes, which may
 *              reach back into earlier segments and overlap p, never past room; under 3, or exactly 3 further than 4096 back, it is no match.  The longest
 *              wins, ties to the smaller distance.
 *   parse      greedy from the segment's start: a match where there is one (skip its length), else a literal.
 *   codes      lengths by Huffman's algorithm: leaves in order of (count, symbol); always join the two smallest of (next leaf, oldest joined node), a leaf
 *              before a node of equal weight.  Deeper than the limit (15; 7 for the code-length code): every used count becomes (count + 1) >> 1 and the tree
 *              is built again.  An alphabet with fewer than two used symbols (a block with one distance code, or none) gives a count of 1 to its lowest unused
 *              symbols until two are used, so every table sent is complete.  Codes are canonical (RFC 1951 3.2.2).
 *   header     HLIT / HDIST are trimmed to the last used symbol (at least 257 / 1); the code lengths are sent ONE BY ONE: the repeat symbols 16, 17, 18 are
 *              not used; HCLEN is trimmed (at least 4). */
typedef enum hive_png_kind { HIVE_PNG_GRAY8 = 0, HIVE_PNG_GRAY16 = 1, HIVE_PNG_RGB8 = 2 } hive_png_kind;
typedef struct hive_png_image {
    const void *pixels; /* device [height][pitch] bytes: width pixels at the start of every row; uint16 samples in host byte order */
    int32_t height, width;
    int64_t pitch;      /* bytes from one row to the next, >= width * bytes per pixel (1, 2, 3) */
    int32_t kind;       /* hive_png_kind */
} hive_png_image;
/* Host only (no context, no device) -> offsets[n], each a multiple of 4, and *total_bytes: room for the WORST case of every file, which is all segments stored:
 * 63 bytes of frame (signature 8, IHDR 25, IDAT's length / type / CRC 12, zlib header 2, Adler-32 4, IEND 12) + the filtered stream H * (1 + row bytes) + 5 per
 * segment of 8192, up to a multiple of 4.  Fails on n < 1, an unknown kind, a side of 0 or above 65535, more than 2^27 stream bytes; the message is
 * hive_last_error(NULL). */
int hive_png_layout(const hive_png_image *images, int n, int64_t *offsets, int64_t *total_bytes);
/* Fourteen launches for any n behind ONE upload of the picture table: file i goes to d_out + offsets[i] (device; out_bytes >= the layout's total, or the call
 * fails naming the bytes needed, before any launch; nothing is ever written past out_bytes), its length to sizes[i] (host).  At most 2^27 bytes of filtered
 * stream per call.  Returns after the device has finished (the sizes come back in one small copy). */
int hive_png_encode(hive_ctx *ctx, const hive_png_image *images, int n, uint8_t *d_out, int64_t out_bytes, int64_t *sizes);

/* ---- depth hand-off DPT -> TSDF ----------------------------------------------------- */
/* dataset_adaptors.py:1432-1433 (x1000 -> uint16 truncation) then io.py:1032-1039
 * (x 1/1000 as float32, > max_depth -> 0), optional mask (non-zero -> depth 0, fusion.py:121).
 * Millimetres outside [0, 65535], where the reference's astype is undefined, saturate: negative -> 0, above -> 65535.
 * in: f32 or f16/bf16 depth in metres [H][W] on the device; out_mm (optional u16) and out_m (f32). */
typedef enum hive_dtype { HIVE_F32 = 0, HIVE_F16 = 1, HIVE_BF16 = 2 } hive_dtype;
int hive_depth_quantize(hive_ctx *ctx, const void *d_depth, int dtype, int H, int W,
                        float depth_scale, float max_depth, const uint8_t *d_mask,
                        uint16_t *d_out_mm, float *d_out_m);

/* ---- DPT ViT encoder blocks: replaces the transformer blocks of dpt.models.DPTDepthModel.forward
 *      (timm vit_base_resnet50_384) -- hive/dataset_adaptors.py:1366-1374,1419 --------------------- */
/* All pointers are device memory.  Activations / weights are the 16-bit type `dtype` names -- HIVE_BF16, or HIVE_F16: what the
 * reference runs (`model.half()` and fp16 samples, hive/dataset_adaptors.py:1394-1401, 1415-1417); same kernels, same rates
 * (v_mfma_f32_16x16x32_{bf16,f16}) -- with [out][in] row-major weights, as nn.Linear stores them; biases and LayerNorm affine
 * parameters are float32.  Below "16-bit" stands for that type. */
typedef struct hive_vit hive_vit;
typedef struct hive_vit_block_weights {
    const void *ln1_g, *ln1_b;   /* f32 [D]            norm1            */
    const void *qkv_w, *qkv_b;   /* 16-bit [3D][D], f32 [3D] attn.qkv   */
    const void *proj_w, *proj_b; /* 16-bit [D][D], f32 [D]   attn.proj  */
    const void *ln2_g, *ln2_b;   /* f32 [D]            norm2            */
    const void *fc1_w, *fc1_b;   /* 16-bit [F][D], f32 [F]   mlp.fc1    */
    const void *fc2_w, *fc2_b;   /* 16-bit [D][F], f32 [D]   mlp.fc2    */
} hive_vit_block_weights;
/* head dim must be 64 (D = 64 * heads), D a multiple of 256 and <= 1024, F a multiple of 128. */
int hive_vit_create(hive_ctx *ctx, int dtype, int depth, int dim, int heads, int mlp_dim, float ln_eps,
                    const hive_vit_block_weights *blocks, hive_vit **out);
/* WEIGHT SNAPSHOT CONTRACT.  hive_vit_create copies what the folded LayerNorm needs -- gamma o W of qkv / fc1 and the constant rows c1 = sum_k (gamma o W)[n][k],
 * c2 = sum_k beta[k] W[n][k] + bias[n] -- into private buffers; proj / fc2 and every bias other than those two are read through the caller's pointers at
 * every forward.  A caller that overwrites weights IN PLACE after create must call hive_vit_weights_modified (re-folds on the context's stream, ordered
 * behind the writes there) before the next forward, or gets old LayerNorm / qkv / fc1 with new proj / fc2.  (hive_dpt: hive_dpt_weights_modified.) */
int hive_vit_weights_modified(hive_vit *vit);
int hive_vit_destroy(hive_vit *vit);
/* x 16-bit [B][N][D] -> runs all blocks; after block tap_blocks[t] its output is copied to tap_out[t]
 * (16-bit [B][N][D]).  x = x + proj(attn(LN1 x)); x = x + fc2(gelu(fc1(LN2 x))). */
int hive_vit_forward(hive_vit *vit, const void *x, int B, int N, const int *tap_blocks, int n_taps,
                     void *const *tap_out);
/* the individual kernels (used by hive_vit_forward; exposed for the numerics tests) */
int hive_vit_layernorm(hive_ctx *ctx, const void *x, int dtype, const float *gamma, const float *beta, void *out,
                       int M, int D, float eps);
/* C = epilogue(A[M][K] W[N][K]^T + bias): epilogue 0 = none, 1 = GELU (erf), 2 = + residual[M][N] */
int hive_vit_linear(hive_ctx *ctx, const void *A, int dtype, const void *W, const float *bias, const void *residual,
                    void *C, int M, int N, int K, int epilogue);
/* qkv projection of x [B*Np][D] (Np a multiple of 64): q|k -> qk [B*Np][2D], v -> vT [B][H][64][Np].  Both are operands
 * private to hive_vit_attention: q is stored multiplied by head_dim^-0.5 * log2(e) (in f32, before the one rounding to 16 bits), so
 * the attention's score products are base-2 exponents; vT is laid out for its fragment reads: along its last axis the token quads 4..7 and 8..11 of every group of 16 are swapped
 * (token t is stored at t with bits 2 and 3 exchanged), which makes the attention's V fragments single 16-byte LDS reads. */
int hive_vit_qkv(hive_ctx *ctx, const void *x, int dtype, const void *W, const float *bias, void *qk, void *vT,
                 int B, int Np, int D, int H);
/* softmax(q k^T / 8) v over the first N keys of each image -> out [B*Np][D]; Np = N rounded up to a multiple of 64; qk, vT as
 * hive_vit_qkv writes them (q pre-scaled: the kernel evaluates exp2(q' k^T - max)).  Where the launch leaves a CU one workgroup at most (one or two 480 x 640
 * frames) each workgroup splits its keys over two groups of waves and merges the halves: another order of float32 additions than at larger batches
 * (hive_ctx_set_deterministic keeps the one-chain form everywhere). */
int hive_vit_attention(hive_ctx *ctx, const void *qk, int dtype, const void *vT, void *out, int B, int N, int Np,
                       int D, int H);

/* ---- DPT pre/post-processing around the network (device pointers) -------------------------------- */
/* uint8 RGB values -> ((x / 255) - mean) / std as f16 / bf16, same element order (a [B][H][W][3] frame
 * batch becomes the channels-last network input) -- hive/dataset_adaptors.py:1407-1417 */
int hive_dpt_preprocess(hive_ctx *ctx, const uint8_t *d_rgb, int64_t n_values, float mean, float std,
                        int dtype, void *d_out);
/* The same for frames that are not the network's size -- hive/dataset_adaptors.py:1376-1389: `dpt.transforms.Resize(net_w, net_h, ...,
 * image_interpolation_method=cv2.INTER_CUBIC)` applied to `image / 255.0`, then NormalizeImage / PrepareForNet / the 16-bit cast:
 * d_rgb u8 [B][H][W][3] -> d_out [B][out_h][out_w][3] in `dtype` (HIVE_F16 / HIVE_BF16; HIVE_F32 for checks).  The output size is the
 * caller's (hive_amd.dpt.transforms.Resize.get_size restates the reference's sizing rule); the arithmetic is cv2.resize's INTER_CUBIC:
 * a = -0.75 cubic, four taps per axis at floor((d + 0.5) * src / dst - 0.5) - 1 .. + 2, indices clamped to the image, no anti-aliasing,
 * float32 weights, rows first.  (cv2 is not available to this build: parity with cv2 itself is unpinned; see csrc/resize.hip.) */
int hive_dpt_resize_preprocess(hive_ctx *ctx, const uint8_t *d_rgb, int B, int H, int W, int out_h, int out_w, float mean, float std,
                               int dtype, void *d_out);
/* hive/dataset_adaptors.py:1421-1426 `torch.nn.functional.interpolate(prediction, size=frame.shape[:2], mode="nearest")` fused with the
 * hand-off of :1432-1433 / hive/io.py:1032-1039: d_depth f32 [B][h][w] -> [B][H][W] outputs (any may be NULL, not all): d_out_depth f32,
 * d_out_mm = uint16(depth * 1000), d_out_m = depth_scale * mm with > max_depth -> 0.  Source index = min((int)floorf(dst * (float)src / dst_size), src - 1). */
int hive_depth_resize_nearest(hive_ctx *ctx, const float *d_depth, int B, int h, int w, int H, int W, float depth_scale, float max_depth,
                              float *d_out_depth, uint16_t *d_out_mm, float *d_out_m);
/* Last layer of the depth head, fused, in float32: 1x1 conv C -> 1 on the channels-last f16 / bf16 map
 * d_feat [n_px][C] (weights / bias on the host), ReLU if non_negative, depth = 1 / max(scale x + shift, 1e-8)
 * if invert (DPTDepthModel.forward).  h_pre_bias (optional, host, [C]) and pre_relu apply the bias and ReLU of the
 * convolution that produced d_feat on the fly (head: conv 128->32 + bias, ReLU, conv 32->1), saving two passes over
 * the largest activation of the network.  Optional outputs: d_depth f32 metres; and the PNG hand-off
 * d_out_mm = uint16(depth * 1000), d_out_m = depth_scale * mm with > max_depth -> 0
 * (hive/dataset_adaptors.py:1432-1433, hive/io.py:1032-1039). */
int hive_dpt_head_tail(hive_ctx *ctx, const void *d_feat, int dtype, int64_t n_px, int C,
                       const float *h_pre_bias, int pre_relu, const float *h_weight, float bias,
                       int non_negative, int invert, float scale, float shift, float *d_depth,
                       float depth_scale, float max_depth, uint16_t *d_out_mm, float *d_out_m);
/* The second half of the depth head as one kernel (f16 / bf16): Interpolate(x2, bilinear, align_corners=True) ->
 * Conv3x3(C_in=128 -> C_mid=32) + bias -> ReLU -> Conv1x1(32 -> 1) + bias -> [ReLU] -> [1 / max(scale x + shift, 1e-8)]
 * -> optional uint16-mm hand-off, i.e. scratch.output_conv[1:] of DPTDepthModel plus the tail above
 * (hive/dataset_adaptors.py:1419, 1432-1433).  d_x: channels-last [N][H][W][C_in] (output of output_conv[0]);
 * d_b0 (optional, device, f32 [C_in]): bias of output_conv[0], added to d_x on load (x + b rounded to the tensor dtype first, as the
 * separate bias add rounds it), so that convolution can run without its bias pass;
 * d_w3: the 3x3 weights on the device as [ky][kx][C_mid][C_in]; h_b3 [C_mid], h_w1 [C_mid] on the host.
 * Outputs are [N][2H][2W]; any of them may be NULL (not all). */
int hive_dpt_head_fused(hive_ctx *ctx, const void *d_x, const float *d_b0, int dtype, int N, int H, int W, int C_in, int C_mid,
                        const void *d_w3, const float *h_b3, const float *h_w1, float b1, int non_negative, int invert,
                        float scale, float shift, float *d_depth, float depth_scale, float max_depth,
                        uint16_t *d_out_mm, float *d_out_m);

/* ---- fused channels-last glue of the DPT convolutional parts (device pointers, f16 / bf16) ----------- */
/* GroupNorm over [N][HW][C] (C a power of two, 8..2048) with G groups, affine gamma / beta [C] in the tensor
 * dtype, optional residual add (same shape) and ReLU:  out = relu?( gn(x) (+ residual) ).  timm GroupNormAct +
 * the bottleneck's `relu(norm3(x) + shortcut)`, reached from DPTDepthModel.forward (dataset_adaptors.py:1419). */
int hive_nhwc_group_norm(hive_ctx *ctx, const void *d_x, int dtype, int N, int HW, int C, int G,
                         const void *d_gamma, const void *d_beta, float eps, const void *d_residual,
                         int relu, void *d_out);
/* out = relu?( (x + bias[c]) (+ residual) (+ residual2) ) over [n_px][C] (C % 8 == 0; bias in the tensor dtype; out may
 * alias x): convolution bias + ReLU + skip adds of the RefineNet residual units / fusion blocks (isl-org/DPT
 * ResidualConvUnit_custom, FeatureFusionBlock_custom) in one pass.  d_out_relu (optional) additionally receives
 * relu(out): the input of the next residual unit's first convolution (its `relu(x)`), saving that unit a pass. */
int hive_nhwc_bias_act(hive_ctx *ctx, const void *d_x, int dtype, int64_t n_px, int C, const void *d_bias, int relu,
                       const void *d_residual, const void *d_residual2, void *d_out, void *d_out_relu);
/* bilinear x2, align_corners=True: [N][H][W][C] -> [N][2H][2W][C] (C % 8 == 0): the RefineNet fusion blocks'
 * and the depth head's `interpolate(scale_factor=2, mode="bilinear", align_corners=True)`.  d_bias (optional, [C], tensor
 * dtype) is added to the input on load, rounded to the tensor dtype first: the bias pass of the producing convolution. */
int hive_nhwc_upsample2x(hive_ctx *ctx, const void *d_in, const void *d_bias, int dtype, int N, int H, int W, int C, void *d_out);

/* 3 x 3 convolution, stride 1, padding 1, channels-last f16 / bf16, as an implicit GEMM on the matrix cores with the decoder's
 * element-wise tail fused:  out = relu?( conv(x, w) (+ bias) (+ residual) (+ residual2) ), and optionally out_relu = relu(out).
 * The 3 x 3 convolutions of isl-org/DPT's decoder reached from DPTDepthModel.forward (hive/dataset_adaptors.py:1419):
 * scratch.layer{1..4}_rn, ResidualConvUnit_custom.conv1 / conv2, scratch.output_conv[0].
 * d_x [N][H][W][C_in]; d_w [C_out][3][3][C_in] (= the [C_out][C_in][3][3] weight tensor in channels-last memory format);
 * d_bias [C_out] in the tensor dtype or NULL; residuals / outputs [N][H][W][C_out].  C_in % 64 == 0, C_out % 128 == 0;
 * the outputs must not alias the input. */
int hive_nhwc_conv3x3(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, const void *d_w,
                      const void *d_bias, int relu, const void *d_residual, const void *d_residual2, void *d_out,
                      void *d_out_relu);

/* The same implicit-GEMM kernel family for the other convolutions of the network (ResNetV2-50 stages of the hybrid backbone --
 * timm StdConv2dSame with its "SAME" padding --, the 1 x 1 projections of the reassemble stages and fusion blocks, the stride-2
 * 3 x 3 of act_postprocess4): kernel 1 or 3 (square), stride 1 or 2, explicit top / left padding (the bottom / right padding
 * is whatever H_out, W_out imply), C_in % 64 == 0, C_out % 64 == 0, d_w [C_out][kernel][kernel][C_in].  Same fused epilogue.
 * Input pixel of tap (ky, kx) for output (oy, ox): (oy * stride + ky - pad_top, ox * stride + kx - pad_left), zero outside. */
int hive_nhwc_conv(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, int kernel, int stride,
                   int pad_top, int pad_left, int H_out, int W_out, const void *d_w, const void *d_bias, int relu,
                   const void *d_residual, const void *d_residual2, void *d_out, void *d_out_relu);

/* The same convolution with the statistics pass of the GroupNorm that follows it (timm ResNetV2: `norm(conv(x))` behind every
 * convolution of the hybrid backbone) folded into the epilogue: per tile of *gn_tile_rows output pixels (all C_out channels) the sum
 * and the sum of squares of the stored outputs, per channel, split between the two samples the tile may touch, are left in
 * d_gn_partial (float, >= hive_nhwc_conv_gn_partial_floats(N * H_out * W_out, C_out) elements).  *gn_tile_rows = 0 when the map is
 * smaller than a tile or the epilogue is more than a store (relu / a residual / d_out_relu given): nothing was written and the
 * GroupNorm makes its own pass.  hive_nhwc_group_norm_stats = hive_nhwc_group_norm
 * taking its statistics from there (d_gn_partial NULL or gn_tile_rows 0: identical to hive_nhwc_group_norm). */
int64_t hive_nhwc_conv_gn_partial_floats(int64_t n_px, int C_out);
int hive_nhwc_conv_gn(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, int kernel, int stride,
                      int pad_top, int pad_left, int H_out, int W_out, const void *d_w, const void *d_bias, int relu,
                      const void *d_residual, const void *d_residual2, void *d_out, void *d_out_relu, void *d_gn_partial,
                      int64_t gn_partial_floats, int *gn_tile_rows);
int hive_nhwc_group_norm_stats(hive_ctx *ctx, const void *d_x, int dtype, int N, int HW, int C, int G, const void *d_gamma,
                               const void *d_beta, float eps, const void *d_residual, int relu, void *d_out,
                               const void *d_gn_partial, int gn_tile_rows);

/* d_out = relu?( GroupNorm_G(conv(x); gamma, beta, eps) (+ d_residual) ) with the convolution's own output never written: the
 * bottleneck tails of timm's ResNetV2 (`norm3(conv3(x))` + shortcut + ReLU, and `downsample.norm(downsample.conv(x))`).  The
 * convolution runs twice -- per-tile channel sums first, then normalisation in the epilogue -- which pays where C_out > C_in.
 * Results are bit-identical to hive_nhwc_conv_gn followed by hive_nhwc_group_norm_stats.  d_scratch: float,
 * >= hive_nhwc_conv_gn_partial_floats(N * H_out * W_out, C_out) + 2 * N * G elements.  *fused = 0: not eligible (needs
 * C_out % 256 == 0, (C_out / G) % 8 == 0, H_out * W_out >= 256), nothing was done and the caller runs the separate sequence. */
int hive_nhwc_conv_gn_apply(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, int kernel,
                            int stride, int pad_top, int pad_left, int H_out, int W_out, const void *d_w, int G,
                            const void *d_gamma, const void *d_beta, float eps, const void *d_residual, int relu, void *d_out,
                            void *d_scratch, int64_t scratch_floats, int *fused);

/* The same for 1 x 1 convolutions (the only kind timm's ResNetV2 uses here) with the GroupNorm's statistics taken from the INPUT instead of a first pass of
 * the convolution: y = W x is linear, so a group's sum is u_g . sum_p x_p and its sum of squares <G_g, sum_p x_p x_p^T> with u_g = sum_{c in g} w_c,
 * G_g = sum_{c in g} w_c w_c^T -- one read of the C_in-wide input and its Gram matrix on the matrix cores (csrc/gram.hip).  hive_gn_gram_prepare makes the
 * tables (hive_gn_gram_table_floats(C_in, G) floats) of a weight tensor [C_out][C_in] once; hive_nhwc_conv_gn_apply_gram then needs d_scratch >= 2 N G floats.
 * These are the statistics of the exact products, not of the 16-bit-rounded outputs: (mean, rstd) agree with the two-pass form to ~1e-4 relative, the
 * outputs to within one rounding in a few places.  *fused = 0: not eligible (hive_nhwc_conv_gn_apply's conditions, C_in in {64, 128, 256}, G % 4 == 0).
 * hive_gn_gram_stats: the statistics alone ([N][G][2] = mean, rstd) and, for tests, the partial Gram matrices [N][parts][C_in][C_in] / sums
 * [N][parts][C_in] (parts = hive_gn_gram_parts(...); d_S_out / d_s_out may be NULL).  Replaces nothing in the reference: an implementation choice behind
 * `norm3(conv3(x))` of /root/reference's DPT-Hybrid backbone (hive/dataset_adaptors.py:1419 runs it). */
int64_t hive_gn_gram_table_floats(int C_in, int G);
int hive_gn_gram_prepare(hive_ctx *ctx, const void *d_w, int dtype, int C_in, int C_out, int G, float *d_tables);
int hive_gn_gram_parts(hive_ctx *ctx, int N, int C_in, int H_out, int W_out);
int hive_gn_gram_stats(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, int stride, int H_out, int W_out, int G,
                       const float *d_tables, float eps, float *d_stats, float *d_S_out, float *d_s_out);
int hive_nhwc_conv_gn_apply_gram(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, int stride, int H_out, int W_out,
                                 const void *d_w, const float *d_tables, int G, const void *d_gamma, const void *d_beta, float eps,
                                 const void *d_residual, int relu, void *d_out, void *d_scratch, int64_t scratch_floats, int *fused);
/* 1 where the statistics from the Gram matrices are the cheaper way for this 1 x 1 convolution (hive_nhwc_conv_gn_apply_gram), 0 where the two-pass form is
 * (hive_nhwc_conv_gn_apply): THE rule of the network object and of the Python orchestration, which stay bit-identical only while they share it.  1 needs
 * all of: hive_nhwc_conv_gn_apply's conditions; G == 32; not deterministic (hive_ctx_set_deterministic: the choice depends on the batch size); the
 * environment's HIVE_GN_GRAM not beginning with '0' (read at every call); and N * H_out * W_out * C_out >= 150 000 000 output elements with C_in 64 or
 * 128, or >= 250 000 000 with C_in == 256 and stride == 2 (below that the Gram path's three small kernels cost more than the first pass they replace).  Pure host
 * code: no context, no device. */
int hive_gn_gram_preferred(int C_in, int C_out, int stride, int G, int N, int H_out, int W_out, int deterministic);

/* DPT-Large (timm vit_large_patch16_384, `DPTDepthModel(backbone="vitl16_384")`) pieces that are not plain convolutions of
 * hive_nhwc_conv:
 *   hive_patch_rows: the patch embedding Conv2d(C, D, P, P) as a GEMM -- the channels-last frame d_x [N][H][W][C] is rearranged into
 *     d_out [N (H/P) (W/P)][P P C] ((ky, kx, c) order = the weight tensor in channels-last memory format); hive_vit_linear with that
 *     weight and the bias then yields the tokens.
 *   hive_nhwc_pixel_shuffle_bias: ConvTranspose2d(C, C, s, s) (reassemble stages 1 and 2) = a 1 x 1 convolution to s s C channels in
 *     (dy, dx, co) order (hive_nhwc_conv) followed by this scatter d_in [N H W][s s C] -> d_out [N][s H][s W][C] (+ d_bias[co]). */
int hive_patch_rows(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C, int patch, void *d_out);
int hive_nhwc_pixel_shuffle_bias(hive_ctx *ctx, const void *d_in, const void *d_bias, int dtype, int N, int H, int W, int C, int s,
                                 void *d_out);

/* ResNetV2 stem of the hybrid backbone (timm 0.5.4 ResNetV2.stem, reached from DPTDepthModel.forward): the 7 x 7 stride-2
 * weight-standardised convolution 3 -> 64 with TensorFlow "SAME" padding on the channels-last frame d_x [N][H][W][3] ->
 * d_out [N][ceil(H/2)][ceil(W/2)][64]; d_w = the standardised weights as [64][7][32] ((kx, c) of a kernel row padded from 21 to
 * 32 with zeros).  And MaxPool2dSame(3, 2): [N][H][W][C] -> [N][ceil(H/2)][ceil(W/2)][C], C % 8 == 0. */
int hive_resnet_stem_conv(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, const void *d_w, void *d_out);
int hive_nhwc_maxpool3x3s2(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C, void *d_out);
/* The stem as the network object runs it (same results as the three calls above with hive_nhwc_group_norm between them):
 * hive_resnet_stem_conv_gn = the convolution, leaving the statistics of the GroupNorm behind it as hive_nhwc_conv_gn does (per 256-pixel
 * tile; d_gn_partial >= hive_nhwc_conv_gn_partial_floats(N * H_out * W_out, 64) floats; *gn_tile_rows = 0 -- nothing written -- unless
 * H_out % 8 == 0 and W_out % 32 == 0); hive_nhwc_group_norm_relu_maxpool = MaxPool2dSame(3, 2)(relu(GroupNorm(x))) in one pass over
 * x [N][H][W][C] -> [N][ceil(H/2)][ceil(W/2)][C] (d_gn_partial / gn_tile_rows as hive_nhwc_group_norm_stats; NULL / 0: own statistics). */
/* t2 = conv2(relu(norm1(t))) of a 64-channel ResNetV2 bottleneck (timm Bottleneck: `x = norm1(conv1(x)); x = norm2(conv2(x))`) as one kernel:
 * d_x [N][H][W][64] is conv1's raw output with the sums its epilogue left (d_in_partial, in_tile_rows: hive_nhwc_conv_gn), d_gamma / d_beta
 * norm1's parameters, d_w conv2's standardised 3 x 3 weights [64][3][3][64]; d_out = conv2's raw output (bit-identical to
 * hive_nhwc_conv on the separately normalised tensor), and the sums of norm2 as hive_nhwc_conv_gn leaves them (d_gn_partial,
 * *gn_tile_rows; 0: none).  *fused = 0 and nothing done where it does not apply (C != 64, no sums from conv1): run the pair. */
int hive_bneck_gn_conv3x3(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C, const void *d_in_partial, int in_tile_rows,
                          const void *d_gamma, const void *d_beta, float eps, const void *d_w, void *d_out, void *d_gn_partial,
                          int64_t gn_partial_floats, int *gn_tile_rows, int *fused);
int hive_resnet_stem_conv_gn(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, const void *d_w, void *d_out, void *d_gn_partial,
                             int64_t gn_partial_floats, int *gn_tile_rows);
int hive_nhwc_group_norm_relu_maxpool(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C, int G, const void *d_gamma,
                                      const void *d_beta, float eps, void *d_out, const void *d_gn_partial, int gn_tile_rows);

/* ---- the whole DPT-Hybrid network behind one handle ------------------------------------------------------------------------
 * dpt.models.DPTDepthModel(path, scale, shift, invert, backbone="vitb_rn50_384", non_negative) + .forward(), with the frame
 * pre-processing and the depth hand-off around it, as HIVE's estimate_depth_dpt uses them (hive/dataset_adaptors.py:1366-1374,
 * 1407-1419, 1432-1433; hive/io.py:1032-1039): uint8 RGB frames in HBM -> depth maps in HBM.
 *
 * The weights come as a table of (name, device pointer).  Names are the parameter names of the published isl-org/DPT checkpoint
 * (`dpt_hybrid_nyu-2ce69ec7.pt`); every tensor is of the config's 16-bit `dtype` unless noted:
 *   pretrained.model.patch_embed.backbone.stem.conv.weight        [64][7][32]: STANDARDISED weights, (ky, (kx, c) padded 21 -> 32)
 *   ...backbone.stem.norm.{weight,bias}, ...stages.S.blocks.B.{norm1,norm2,norm3,downsample.norm}.{weight,bias}     [C]
 *   ...stages.S.blocks.B.{conv1,conv2,conv3,downsample.conv}.weight   [C_out][k][k][C_in]: STANDARDISED (timm StdConv2dSame, eps 1e-8)
 *   pretrained.model.patch_embed.proj.{weight [768][1][1][1024], bias [768]},  pretrained.model.cls_token [768]
 *   pretrained.model.blocks.I.{norm1,norm2}.{weight,bias} f32 [768]; attn.qkv.weight [2304][768], attn.qkv.bias f32; attn.proj.*;
 *   mlp.fc1.weight [3072][768], mlp.fc1.bias f32; mlp.fc2.weight [768][3072], mlp.fc2.bias f32            (I = 0 .. 11)
 *   pretrained.act_postprocess{3,4}.0.project.0.{weight [768][1536], bias f32 [768]}
 *   pretrained.act_postprocess3.3.*, act_postprocess4.3.* ([768][1][1][768] + bias), act_postprocess4.4.* ([768][3][3][768] + bias)
 *   scratch.layer{1..4}_rn.weight [256][3][3][C_in];  scratch.refinenet{1..4}.resConfUnit{1,2}.conv{1,2}.{weight [256][3][3][256], bias};
 *   scratch.refinenet{1..4}.out_conv.{weight [256][1][1][256], bias}
 *   scratch.output_conv.0.{weight [128][3][3][256], bias [128]}; scratch.output_conv.2.weight as
 *   [ky][kx][32][128]; the last two layers' host values go in the config (head_b3 = output_conv.2.bias, head_w1 / head_b1 = output_conv.4).
 * All convolution weights are [C_out][ky][kx][C_in] (= the PyTorch tensor in channels-last memory format).  The pointers must
 * stay valid for the life of the handle.
 * backbone 1 (DPT-Large, `dpt_large-midas-2f21e586.pt`: no ResNet; 24 blocks of width 1024, hooks 5 / 11 / 17 / 23) differs in:
 *   pretrained.model.patch_embed.proj.weight [1024][16][16][3] (the GEMM's [1024][768]), ...proj.bias.f32 (f32 [1024]), cls_token [1024];
 *   blocks.I.* with 768 -> 1024, 3072 -> 4096 (I = 0 .. 23); act_postprocess{1..4}.0.project.0.{weight [1024][2048], bias f32};
 *   act_postprocess1.3.* [256][1][1][1024], act_postprocess1.4.weight.rows [4 4 256][256] = ConvTranspose2d(256, 256, 4, 4).weight
 *   permuted to ((dy, dx, co), ci), act_postprocess1.4.bias; act_postprocess2.3.* [512][1][1][1024], act_postprocess2.4.weight.rows
 *   [2 2 512][512], .bias; act_postprocess3.3.* [1024][1][1][1024]; act_postprocess4.3.* likewise, act_postprocess4.4.* [1024][3][3][1024];
 *   scratch.layer{1..4}_rn.weight with C_in = 256 / 512 / 1024 / 1024. */
typedef struct hive_dpt hive_dpt;
typedef struct hive_dpt_tensor {
    const char *name;
    const void *data;
} hive_dpt_tensor;
typedef struct hive_dpt_config {
    int backbone;                 /* 0 = vitb_rn50_384 (DPT-Hybrid: the one HIVE instantiates), 1 = vitl16_384 (DPT-Large) */
    float scale, shift;           /* depth = 1 / max(scale * x + shift, 1e-8) when invert */
    int invert, non_negative;
    float gn_eps, ln_eps;         /* 1e-5 (GroupNorm), 1e-6 (timm ViT LayerNorm) */
    float head_b3[32], head_w1[32], head_b1;
    int dtype;                    /* HIVE_BF16 or HIVE_F16: the type of every 16-bit tensor of the table, of d_pos_embed and of the activations */
} hive_dpt_config;
int hive_dpt_create(hive_ctx *ctx, const hive_dpt_config *config, const hive_dpt_tensor *tensors, int n_tensors, hive_dpt **out);
/* d_rgb u8 [B][H][W][3] (H, W multiples of 32), d_pos_embed (the config's dtype) [(H/16)(W/16) + 1][768 | 1024] = the position embedding resized to this
 * token grid (dpt `_resize_pos_embed`: evaluated once per frame size by the host binding).  Outputs [B][H][W], any may be NULL (not
 * all): d_depth f32 metres; d_out_mm = uint16(depth * 1000); d_out_m = mm / 1000 with > max_depth -> 0. */
int hive_dpt_forward(hive_dpt *dpt, const uint8_t *d_rgb, int B, int H, int W, const void *d_pos_embed, float *d_depth, float max_depth,
                     uint16_t *d_out_mm, float *d_out_m);
/* Frames of ANY size (BASELINE config 4: 1920 x 1080): d_rgb u8 [B][frame_h][frame_w][3] enters through hive_dpt_resize_preprocess at the network's
 * net_h x net_w (multiples of 32; the reference's rule gives 864 x 480 for 1080p, hive/dataset_adaptors.py:1376-1389), the depth map leaves through
 * hive_depth_resize_nearest at the frame size (:1421-1426): outputs [B][frame_h][frame_w].  d_pos_embed is the embedding of the NETWORK's token grid
 * (net_h / 16)(net_w / 16) + 1.  With net == frame size this is hive_dpt_forward. */
int hive_dpt_forward_frames(hive_dpt *dpt, const uint8_t *d_rgb, int B, int frame_h, int frame_w, int net_h, int net_w, const void *d_pos_embed,
                            float *d_depth, float max_depth, uint16_t *d_out_mm, float *d_out_m);
/* The activation arena a forward of these shapes needs, without a device: every forward first PLANS -- walks the network's allocation sequence (each map
 * allocated from shapes alone, released behind its last consumer, first fit over the freed blocks) -- reserves *bytes, the plan's high-water mark, and then
 * launches over that memory repeating the same sequence.  A launch walk that asks for a block ending beyond the plan launches nothing with it: the forward
 * returns HIVE_ERR_STATE, as it does when it ends with another size than planned.  hive_dpt_forward_frames sizes its arena through this very walk.
 * backbone as hive_dpt_config; the argument checks of hive_dpt_forward_frames.  *layout_hash (may be NULL): 64-bit FNV-1a (basis 0xcbf29ce484222325, prime
 * 0x100000001b3) over the (offset, bytes) of every allocation in order, each as 8 little-endian bytes: it fixes the layout, not only its size.  Pure host
 * code: no context. */
int hive_dpt_plan_arena(int backbone, int B, int frame_h, int frame_w, int net_h, int net_w, int64_t *bytes, uint64_t *layout_hash);
/* Bytes of the activation arena (grown to the largest plan seen: the high-water mark of its maps, which are released behind
 * their last consumer -- ~10 GB for 96 frames of 480 x 640, where the maps total 38 GB). */
int hive_dpt_arena_bytes(hive_dpt *dpt, int64_t *bytes);
/* The table's tensors were overwritten in place: refresh what the object derived from them -- the ViT engine's folded LayerNorm weights (captured at
 * hive_dpt_create, see hive_vit_weights_modified) and the Gram tables of the bottlenecks' 1 x 1 convolutions (made on the first forward that needs them).
 * Everything else is read through the table's pointers at every forward.  Pointers must stay the same; new tensors need a new object. */
int hive_dpt_weights_modified(hive_dpt *dpt);
int hive_dpt_destroy(hive_dpt *dpt);

#ifdef __cplusplus
}
#endif
#endif /* HIVE_MI355X_H */
