/*
 * flux3d_hip.h -- C ABI of libflux3d_hip.so: the MI355X (gfx950) implementation of Flux3D.jl's
 * batched geometric-metric hot path.
 *
 * The reference (FluxML/Flux3D.jl, pure Julia) has no FFI; its only device seam is Julia
 * dispatch on array storage type (src/metrics/pcloud.jl:54 vs :72, TriMesh{T,R,S}
 * src/rep/mesh.jl:70).  This header is what a `@ccall` shim binds to replace the CuArray methods
 * (julia/Flux3DHip.jl; INTEGRATION.md shows the binding).  Each entry point cites the
 * reference function it replaces.
 *
 * Conventions
 *   - every function returns fx3d_status (0 = ok, <0 = error); text via fx3d_last_error().
 *     No exceptions cross the boundary.  The shim turns non-zero into `error(msg)`, matching the
 *     reference's error()/DimensionMismatch style (src/rep/pcloud.jl:37-38).
 *   - layouts are exactly Julia's column-major arrays: a point batch (D,N,B) Float32 is the
 *     contiguous stream x[(b*N+i)*D+d]; index outputs are int32, 0-based (the shim adds 1 and
 *     builds CartesianIndex), shaped (N,B).
 *   - pointers named *_dev / documented "device" are device pointers (from fx3d_malloc or any
 *     HIP allocation of the same process, e.g. a torch tensor's data_ptr); "host" are host.
 *   - alignment: every array argument needs the alignment of its ELEMENT TYPE and no more -- 4 bytes for const float * /
 *     int32_t * / uint32_t *, 8 for int64_t * / uint64_t * / double *, 1 for uint8_t * -- so a batch shard of an odd-N cloud
 *     (x + 3 N b), a column range of a packed mesh (v + 3 off), a slice of a flat parameter or gradient buffer (p + at), a Julia
 *     view or a torch slice are valid arguments as they are.  Results do not depend on the pointers' low bits: where a kernel has
 *     a 16-byte path it is chosen from the address and its scalar twin gives the same bits (DESIGN.md 2.1 lists every such site
 *     and the test that holds it).  The exceptions, each refused before any launch:
 *       workspaces (`ws`)            scratch is laid out from the pointer as given: pass fx3d_malloc's alignment (256 bytes).
 *                                    The model entry points check it -- 16 bytes for fx3d_pointnet_forward / _forward_train,
 *                                    256 bytes for the others -- and answer FX3D_ERR_INVALID_ARG; fx3d_knn_ws takes a
 *                                    workspace that is not 256-byte aligned as no workspace (it then is fx3d_knn);
 *       x1 of fx3d_dgcnn_forward /
 *       fx3d_dgcnn_forward_train     16 bytes: FX3D_ERR_INVALID_ARG.
 *     (fx3d_knn_ws builds its pre-pass image only for 16-byte aligned clouds; others run the kernels of fx3d_knn: same results.)
 *   - the caller owns every buffer; the library keeps no pointer past return.
 *   - ops are asynchronous on `stream` (NULL = the device's default stream) unless they have a
 *     host output, which makes them synchronise that stream before returning.
 *   - scratch is caller-provided: query the size with the matching *_workspace_bytes().  A workspace is recycled memory of exactly
 *     that size: its contents on entry are ARBITRARY (a call reads no workspace word that it, or the documented earlier call of its
 *     pair, has not written; results do not depend on what the bytes held), and no byte at or after ws + the queried size is
 *     written.  What a workspace carries from one call to the next, same ws, same sizes, same stream, nothing else run on it in
 *     between: fx3d_voxel_mesh_count -> _emit;  fx3d_edges_dev_count -> _emit;  fx3d_sample_points_cdf / _cdf_pair -> _draw /
 *     _draw_pair / _draw_pair_reg (the CDF; it stays valid while the vertices do);  fx3d_mesh_losses -> fx3d_mesh_losses_bwd with
 *     reuse_forward != 0, and fx3d_mesh_reg.ws from fx3d_sample_points_draw_pair_reg to fx3d_chamfer_sampled_bwd_step_reg (the
 *     Laplacian's unit rows).  fx3d_chamfer_sums -> fx3d_chamfer_finalize[_many] carry sums_dev, not the workspace.  Nothing else
 *     survives a call.  A workspace that is NULL where the query is positive, or shorter than the query, is refused before any
 *     device work, outputs and workspace untouched: FX3D_ERR_WORKSPACE by the chamfer entry points (fx3d_chamfer_sums, _fwd,
 *     _fwd_bwd, _fwd_sharded[_async], _loss_pairwise_f32, _sampled_bwd[_step[_reg]]), fx3d_segment_minmax, fx3d_normalize, the
 *     normals adjoints, fx3d_index_upload, the mesh losses (fx3d_edge_loss, fx3d_laplacian_loss, fx3d_mesh_losses[_bwd],
 *     fx3d_mesh_reg.ws) and the sampler (fx3d_sample_points[_cdf[_pair] / _draw[_pair[_reg]]]); FX3D_ERR_INVALID_ARG by the
 *     models (PointNet, DGCNN, EdgeConv: every entry point), the device topology builders (fx3d_edges_dev_*,
 *     fx3d_laplacian_dev_csr, fx3d_vertex_faces_dev, fx3d_faces_padded_to_packed_dev) and the voxel entry points
 *     (fx3d_pointcloud_to_voxel, fx3d_trimesh_to_voxel, fx3d_voxel_mesh_count / _emit).  Two entry points fall back instead, with
 *     the same results: fx3d_knn_ws (it then is fx3d_knn) and the pruned tier of the chamfer forward (see
 *     fx3d_chamfer_workspace_bytes).  DESIGN.md 2.2 lists every entry point and the test that holds it.
 *   - floating point is Float32 without fused multiply-add on the result-defining path
 *     (distance, area, sampling), so results are bit-identical to the CPU restatement.
 */
#ifndef FLUX3D_HIP_H
#define FLUX3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FX3D_API __attribute__((visibility("default")))

typedef int32_t fx3d_status;
#define FX3D_OK 0
#define FX3D_ERR_INVALID_ARG (-1) /* bad shape / null pointer / unsupported size */
#define FX3D_ERR_HIP (-2)         /* a HIP runtime call failed (text in fx3d_last_error) */
#define FX3D_ERR_OOM (-3)
#define FX3D_ERR_NO_DEVICE (-4)   /* no gfx950 device visible */
#define FX3D_ERR_UNSUPPORTED (-5)
#define FX3D_ERR_WORKSPACE (-6)   /* workspace pointer null or too small */
#define FX3D_ERR_RCCL (-7)        /* librccl missing or an RCCL call failed */

typedef void *fx3d_stream_t; /* hipStream_t */
typedef void *fx3d_event_t;  /* hipEvent_t  */
typedef void *fx3d_comm_t;   /* ncclComm_t (RCCL) */
typedef void *fx3d_multi_t;  /* the communicators + worker threads of several devices of ONE process (fx3d_comm_init_all) */

/* ---- library / device management (replaces Flux3D.use_cuda + CUDA.jl plumbing,
 *      src/Flux3D.jl:52-61; `gpu`/`cpu` functor walkers src/rep/pcloud.jl:57) -------------- */
FX3D_API const char *fx3d_version(void);
FX3D_API size_t fx3d_last_error(char *buf, size_t n); /* thread-local message; returns strlen */

/* ---- variant switches --------------------------------------------------------------------------------------------
 * The kernels' alternative code paths (A/B measurements, tests) are chosen by named integer options, process-wide and
 * atomic -- twelve since round 6: nn1_variant (3 | 0), nn1_nosplit, bwd_global_atomics, knn_no_mfma, knn_no_prepass,
 * knn_slices, edgeconv_unfused, lap_bwd_scatter, cdf_multiblock_from, nn1_tiny_mpairs, mesh_max_blocks, nn1_prune (1 | 0:
 * the spatial pruning of the fp16 nearest-neighbour kernel, which needs the larger workspace fx3d_chamfer_workspace_bytes
 * reports while it is on) (fx3d_option_count / fx3d_option_name enumerate them).  The environment variables FX3D_<NAME> only seed the defaults,
 * once, at the first use of the library; no entry point reads the environment on its launch path.  A host that runs two
 * configurations in one process sets the option before the calls that need it. */
FX3D_API fx3d_status fx3d_set_option(const char *name, int32_t value);
FX3D_API fx3d_status fx3d_get_option(const char *name, int32_t *value);
FX3D_API int32_t fx3d_option_count(void);
FX3D_API const char *fx3d_option_name(int32_t index); /* NULL past the end */
FX3D_API fx3d_status fx3d_device_count(int32_t *n);
FX3D_API fx3d_status fx3d_set_device(int32_t dev);
FX3D_API fx3d_status fx3d_get_device(int32_t *dev);
FX3D_API fx3d_status fx3d_device_name(int32_t dev, char *buf, size_t n);
/* Which physical device `dev` is: its PCI bus id ("0000:c5:00.0", hipDeviceGetPCIBusId) and the 16 bytes of its UUID
 * (hipDeviceProp_t::uuid) -- what a multi-process run gathers per rank to PROVE that N ranks sat on N devices
 * (bench.py `comm.ranks`; the reference has no multi-device code). */
FX3D_API fx3d_status fx3d_device_identity(int32_t dev, char *pci_bus_id, size_t n, uint8_t *uuid16);
FX3D_API fx3d_status fx3d_device_sync(void);
FX3D_API fx3d_status fx3d_malloc(void **dev_ptr, size_t bytes);
FX3D_API fx3d_status fx3d_free(void *dev_ptr);
/* Capture and replay.  Every entry point that takes a stream carries a Capture note: `replayed` -- it may be recorded by
 * fx3d_graph_begin_capture / _end_capture on a created stream and replayed, after one eager call of the same sequence (the library
 * sets its arrival counters and per-kernel attributes up on eager calls); a recorded call has its addresses and host arguments
 * frozen, finds in its workspace what the last replay left, and a host pointer it takes (loss_host) must be NULL; or the reason it
 * cannot be recorded: `copies to the host` (it synchronises), `host code` (it enqueues no work of its own: stream and graph
 * management), `collective` (RCCL; not attempted).  tests/test_gpu_replay.py holds every `replayed` one to its reference as a
 * replayed graph.
 * Capture: fx3d_memcpy_h2d, fx3d_memcpy_d2h: copies to the host -- pageable host memory, the call waits for the copy.
 * fx3d_memcpy_d2d, fx3d_memset, fx3d_counter_add: replayed.  fx3d_stream_destroy, fx3d_stream_sync, fx3d_graph_begin_capture,
 * fx3d_graph_end_capture, fx3d_graph_launch, fx3d_event_record, fx3d_stream_wait_event: host code -- the capture's own machinery
 * (record and wait are the fork and join of a capture over two streams). */
FX3D_API fx3d_status fx3d_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_memset(void *dst_dev, int32_t byte, size_t bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_stream_create(fx3d_stream_t *s);
FX3D_API fx3d_status fx3d_stream_destroy(fx3d_stream_t s);
FX3D_API fx3d_status fx3d_stream_sync(fx3d_stream_t s);
/* Stream capture (hipGraph): record everything enqueued on `s` between begin and end, replay it with one launch.
 * No reference counterpart (the reference runs op by op through CUDA.jl); it serves the launch-bound fit_mesh
 * iteration (examples/fit_mesh.jl:98-110).  Capture needs a created stream; the captured calls must not allocate
 * through hipMalloc-synchronising paths or copy to the host (warm the loop up once before capturing). */
typedef void *fx3d_graph_t; /* opaque: the instantiated hipGraphExec_t and the hipGraph_t it came from, kept alive with it */
FX3D_API fx3d_status fx3d_graph_begin_capture(fx3d_stream_t s);
FX3D_API fx3d_status fx3d_graph_end_capture(fx3d_stream_t s, fx3d_graph_t *g);
FX3D_API fx3d_status fx3d_graph_launch(fx3d_graph_t g, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_graph_destroy(fx3d_graph_t g);
/* *ctr += inc on the device, stream ordered: the per-replay part of a sampling seed (fx3d_sample_points_draw). */
FX3D_API fx3d_status fx3d_counter_add(uint64_t *ctr, uint64_t inc, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_event_create(fx3d_event_t *e);
/* An event for ordering only (fx3d_stream_wait_event between streams of ONE device, fx3d_event_sync from the host): no
 * timestamps (fx3d_event_elapsed_ms is an error on it) and no system-scope fence at the record -- cheaper on the device. */
FX3D_API fx3d_status fx3d_event_create_sync(fx3d_event_t *e);
FX3D_API fx3d_status fx3d_event_destroy(fx3d_event_t e);
FX3D_API fx3d_status fx3d_event_record(fx3d_event_t e, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_event_sync(fx3d_event_t e);
/* Work enqueued on `s` after this call starts only once `e` has completed (device-side ordering, no host wait). */
FX3D_API fx3d_status fx3d_stream_wait_event(fx3d_stream_t s, fx3d_event_t e);
FX3D_API fx3d_status fx3d_event_elapsed_ms(fx3d_event_t start, fx3d_event_t stop, float *ms);

/* ---- kernel timing hooks (the reference has no tracing; BenchmarkTools/CUDA.@sync
 *      in benchmarks/metrics.jl:27-31,82 is what this replaces).  When enabled, every op brackets
 *      its DOMINANT kernel launch with HIP events on the op's own stream; stats are per kernel name
 *      ("nn1", "knn", "sample", "edge_loss", "laplacian_loss", "faces_areas", ...).  Reading the
 *      stats synchronises the recorded events.  Up to 8192 launches are kept per enable. ---- */
FX3D_API fx3d_status fx3d_profile_enable(int32_t every_nth); /* 0 = off, 1 = every launch, n = every n-th; resets */
FX3D_API fx3d_status fx3d_profile_kernel_stats(const char *name, double *avg_ms, double *min_ms,
                                               double *max_ms, int64_t *count);

/* ---- nearest neighbours + chamfer (src/metrics/pcloud.jl) ----------------------------------
 * fx3d_nn1 replaces _nearest_neighbors(::CuArray{Float32,3}, ::CuArray{Float32,3})
 * (src/metrics/pcloud.jl:72-86) with the *CPU method's* semantics (:54-70): exact Float32
 * direct-difference distance, lowest index on ties.  x:(D,N,B) y:(D,M,B) device.
 * idx_x:(N,B) int32 0-based index into y ; idx_y:(M,B) into x ; dmin_* squared distances.
 * Any of the four outputs may be NULL. */
/* Capture: fx3d_nn1: replayed. */
/* Batch axis: fx3d_nn1: B <= 536870911 -- the batch lies on the grid's x; B * 2 * ceil(max(N, M) / 256) < 2^30 is all that binds it. */
FX3D_API fx3d_status fx3d_nn1(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                              int32_t D, int32_t *idx_x, int32_t *idx_y, float *dmin_x,
                              float *dmin_y, fx3d_stream_t s);

/* The launch plan fx3d_nn1 / fx3d_chamfer_* take for this problem size on the current device, as text (kernel variant,
 * candidates per LDS image, chunk subsets per query tile, query passes per block, query tiles, grid, queries per thread R,
 * and last the kernel: f16, tiny, small_d or generic): for tools and bug reports. */
/* Batch axis: fx3d_nn1_plan_describe: unbounded -- a host query; it does not apply the entry points' limit. */
FX3D_API fx3d_status fx3d_nn1_plan_describe(int32_t N, int32_t M, int32_t B, int32_t D, char *buf, size_t n);

/* Scratch needed by the chamfer entry points below (bytes).  While nn1_prune is on, a shape that takes the pruned launch asks for
 * the blocks' scratch on top of the partial sums: 16-bit point indices, two bytes per candidate and per query of a block's window
 * (2.7 MB at B = 32, N = M = 4096).  A workspace of at least this size runs pruned, a smaller one that still holds the partial
 * sums (the size reported with nn1_prune = 0) runs unpruned; both give the same indices. */
/* Batch axis: fx3d_chamfer_workspace_bytes: unbounded -- a host query; it does not apply the entry points' limit. */
FX3D_API fx3d_status fx3d_chamfer_workspace_bytes(int32_t N, int32_t M, int32_t B, int32_t D,
                                                  size_t *bytes);

/* Partial sums of _chamfer_distance (src/metrics/pcloud.jl:47-48) for this batch (shard):
 *   sums_dev[0] = sum_b sum_i ||x_i - y_nn(i)||^2 ,  sums_dev[1] = sum_b sum_j ||y_j - x_nn(j)||^2
 * (double, device, deterministic reduction order).  idx_x/idx_y optional (NULL to skip). */
/* Capture: fx3d_chamfer_sums, fx3d_chamfer_finalize, fx3d_chamfer_finalize_many: replayed. */
/* Batch axis: fx3d_chamfer_sums: B <= 536870911 -- as fx3d_nn1.  The split plan's two-launch form (few clouds of many thousands of
 * points) has both directions of every cloud on the grid's y and refuses B > 32767 before any launch; no shape with that many
 * clouds plans it today. */
FX3D_API fx3d_status fx3d_chamfer_sums(const float *x, int32_t N, const float *y, int32_t M,
                                       int32_t B, int32_t D, double *sums_dev, int32_t *idx_x,
                                       int32_t *idx_y, void *ws, size_t ws_bytes,
                                       fx3d_stream_t s);

/* loss = w1 * (Float32(sums[0]/(D*N*Bg)) * 3f0) + w2 * (Float32(sums[1]/(D*M*Bg)) * 3f0)
 * (src/metrics/pcloud.jl:47-50; the hard-coded 3.0f0 is kept for D != 3).  The sums are Float64 accumulations of the
 * Float32 squared distances, rounded to Float32 once; the reference's `mean` is a Float32 pairwise sum: the two differ
 * by O(log2(n) 2^-24) relative, inside north_star's 1e-5 (the oracle defines the loss the same way).  Bg is the GLOBAL batch
 * size: after an all-reduce(sum) of sums_dev over the ranks that sharded the batch, every rank
 * calls this with the same Bg.  loss_dev: device float. */
FX3D_API fx3d_status fx3d_chamfer_finalize(const double *sums_dev, int32_t N, int32_t M,
                                           int64_t B_global, int32_t D, float w1, float w2,
                                           float *loss_dev, fx3d_stream_t s);
/* The same for `count` evaluations at once: sums_dev (2,count), losses_dev (count).  An evaluation loop over
 * many sharded batches (ModelNet-style eval, BASELINE config 5) keeps one sums slot per batch, all-reduces them
 * with ONE collective per `count` batches and finalises them here. */
FX3D_API fx3d_status fx3d_chamfer_finalize_many(const double *sums_dev, int32_t count, int32_t N, int32_t M,
                                                int64_t B_global, int32_t D, float w1, float w2,
                                                float *losses_dev, fx3d_stream_t s);

/* ---- PointCloud / TriMesh transforms (src/transforms/pcloud_func.jl, src/transforms/mesh_func.jl:99-399) ----------------
 * Segments: x is a (D, ncols) column-major Float32 stream of B segments.  seg_off == NULL: DENSE (D, n_max, B), segment b is
 * columns [b n_max, (b+1) n_max) (a PointCloud).  Otherwise PACKED: seg_off is a device int64 array of B+1 prefix sums of the
 * per-mesh vertex counts, segment b is columns [seg_off[b], seg_off[b+1]), and n_max is the longest segment (a TriMesh's
 * (3, sum V), n_max = Vmax).  Outputs have the input's shape; y == x is allowed.
 * Statistics of normalize, the contract (the reference's own orders -- a sequential Float32 chain on the CPU, another tree
 * with CUDA -- are not targets): over the n real points of a segment (n = N for a cloud, n = verts_len[b] for a mesh; the
 * reference's `_correction` only undoes its zero padding),
 *   c = Float32(sum x / n)  with the sum in Float64,
 *   s = Float32(sqrt(sum (x - c)^2 / (n - 1)))  in Float64, with c the Float32 centroid (the reference passes it as `mean =`).
 * The device result is within 1 ulp of these values and is the same bits on every run: the summation order is a function
 * of (D, n_max, B) alone (per-chunk Float64 sums and centred sums, a fixed block tree, no float atomics).  n = 1 gives
 * s = NaN (0/0), and so NaN output, in both forms, like the reference.
 * Plan (fx3d_transform_plan_describe): chunk = 16384 / D columns; nchunks = ceil(n_max / chunk).  nchunks <= 1: FUSED, one
 * block per segment, statistics and map in one launch, no workspace.  Otherwise TWO LAUNCHES: per-chunk partials into ws
 * (fx3d_transform_workspace_bytes), then a map launch that folds its segment's partials.  No host synchronisation: every
 * entry point can be captured into a graph.  D <= 1024 for normalize, realign and segment_minmax. */
#define FX3D_NORMALIZE_EPS_ADD 0 /* PointCloud: (x - c) / (s + EPS)            src/transforms/pcloud_func.jl:16-22 */
#define FX3D_NORMALIZE_EPS_MAX 1 /* TriMesh:    (x - c) / max(s, EPS), Julia's max (NaN wins)   mesh_func.jl:99-113 */
#define FX3D_SCALE 0             /* y = factor * x       (lmul!, pcloud_func.jl:62-66, mesh_func.jl:154-160) */
#define FX3D_TRANSLATE 1         /* y = x + t[row]       (mesh_func.jl:331-339), D = 3 */
/* Capture: fx3d_segment_minmax, fx3d_normalize, fx3d_realign, fx3d_rotate, fx3d_scale_translate: replayed -- the host vectors
 * (scale, translation, one rotation matrix) are read while recording. */
/* Batch axis: fx3d_transform_plan_describe, fx3d_transform_workspace_bytes, fx3d_segment_minmax, fx3d_normalize, fx3d_realign,
 * fx3d_rotate: B <= 65535 -- a segment is a row of the grid's y; refused by the argument check, the queries included. */
FX3D_API fx3d_status fx3d_transform_plan_describe(int32_t D, int64_t n_max, int32_t B, char *buf, size_t n);
FX3D_API fx3d_status fx3d_transform_workspace_bytes(int32_t D, int64_t n_max, int32_t B, size_t *bytes);
/* minimum / maximum(x, dims = 2) per segment with Julia's min / max (NaN propagates, min(-0.0, 0.0) = -0.0,
 * max(-0.0, 0.0) = 0.0): min_out, max_out (D, B) device.  pad_zero != 0: every segment shorter than n_max also takes +0.0
 * into both (realign!(::TriMesh) reduces over verts_padded, mesh_func.jl:281-283).  n_max == 0 is an error (Julia throws on
 * an empty reduction, pcloud_func.jl:215-216).  ws: fx3d_transform_workspace_bytes. */
FX3D_API fx3d_status fx3d_segment_minmax(const float *x, int32_t D, int64_t n_max, int32_t B, const int64_t *seg_off,
                                         int32_t pad_zero, float *min_out, float *max_out, void *ws, size_t ws_bytes,
                                         fx3d_stream_t s);
/* normalize! (pcloud_func.jl:16-22 with mode EPS_ADD, mesh_func.jl:99-113 with mode EPS_MAX): y = (x - c) / (s + EPS) or
 * (x - c) / max(s, EPS), c and s per (row, segment) as stated above.  centroid_out, scale_out: optional (D, B) device copies
 * of c and s.  ws: fx3d_transform_workspace_bytes. */
FX3D_API fx3d_status fx3d_normalize(const float *x, int32_t D, int64_t n_max, int32_t B, const int64_t *seg_off, int32_t mode,
                                    float *y, float *centroid_out, float *scale_out, void *ws, size_t ws_bytes, fx3d_stream_t s);
/* realign! (pcloud_func.jl:206-218, mesh_func.jl:276-289): y = ((x - smin) / ((smax - smin) + EPS)) * (tmax - tmin) + tmin,
 * unfused, in that bracketing; src_min / src_max (D, B) device (fx3d_segment_minmax), tgt_min / tgt_max (D) device. */
FX3D_API fx3d_status fx3d_realign(const float *x, int32_t D, int64_t n_max, int32_t B, const int64_t *seg_off,
                                  const float *src_min, const float *src_max, const float *tgt_min, const float *tgt_max,
                                  float *y, fx3d_stream_t s);
/* rotate! (pcloud_func.jl:120-137, mesh_func.jl:221-235): y[:, j] = transpose(R) * x[:, j] with D = 3, evaluated as
 * y_i = (R[0,i] x0 + R[1,i] x1) + R[2,i] x2 in Float32, unfused, in that order (R column-major, R[k,i] at k + 3 i).  The
 * reference goes through BLAS (`*`, batched_mul), whose order is not pinned.  Exactly one of: rotmat_host, 9 floats read during
 * the call (one matrix for the whole batch, passed to the kernel by value); rotmat_dev, (3, 3, B) device, the matrix of each
 * column's segment.  ncols: columns of x (dense: n_max * B). */
FX3D_API fx3d_status fx3d_rotate(const float *x, int64_t ncols, int64_t n_max, int32_t B, const int64_t *seg_off,
                                 const float *rotmat_host, const float *rotmat_dev, float *y, fx3d_stream_t s);
/* scale! / translate! over a flat stream of n floats (pcloud_func.jl:62-66, mesh_func.jl:154-160, 331-339): mode FX3D_SCALE,
 * y = vec_host[0] * x; mode FX3D_TRANSLATE, y[i] = x[i] + vec_host[i % 3] (D = 3, n % 3 == 0).  vec_host is read during the
 * call and passed to the kernel by value.  Argument checks on factor and vector are the caller's (the reference's errors). */
FX3D_API fx3d_status fx3d_scale_translate(const float *x, int64_t n, int32_t mode, const float *vec_host, float *y,
                                          fx3d_stream_t s);

/* _chamfer_distance(A,B,w1,w2) forward in one call (src/metrics/pcloud.jl:39-52). loss_dev
 * device float; loss_host optional host float (non-NULL => stream is synchronised). */
/* Capture: fx3d_chamfer_fwd, fx3d_chamfer_bwd: replayed -- fx3d_chamfer_fwd with loss_host NULL (a loss_host makes it wait for a
 * copy to the host). */
/* Batch axis: fx3d_chamfer_fwd, fx3d_chamfer_bwd: B <= 536870911 -- as fx3d_nn1 (fx3d_chamfer_fwd: and as fx3d_chamfer_sums). */
FX3D_API fx3d_status fx3d_chamfer_fwd(const float *x, int32_t N, const float *y, int32_t M,
                                      int32_t B, int32_t D, float w1, float w2, float *loss_dev,
                                      float *loss_host, int32_t *idx_x, int32_t *idx_y,
                                      void *ws, size_t ws_bytes, fx3d_stream_t s);

/* Zygote adjoint of src/metrics/pcloud.jl:47-48 with indices constant (@ignore, :45):
 *   gx = gout*w1*6/(D*N*Bg) * (x - y[idx_x])  - scatter_add_{idx_y}(gout*w2*6/(D*M*Bg)*(y - x[idx_y]))
 *   gy symmetric.   gx:(D,N,B) gy:(D,M,B) device, overwritten. */
FX3D_API fx3d_status fx3d_chamfer_bwd(const float *x, int32_t N, const float *y, int32_t M,
                                      int32_t B, int32_t D, const int32_t *idx_x,
                                      const int32_t *idx_y, float w1, float w2, float gout,
                                      int64_t B_global, float *gx, float *gy, fx3d_stream_t s);

/* Value and gradient of _chamfer_distance in ONE call -- the shape of `gradient(() -> chamfer_distance(A, B), ...)`
 * (benchmarks/metrics.jl:24-38 "total", examples/fit_mesh.jl:106-110): fx3d_chamfer_fwd (loss with the batch size B_global)
 * and fx3d_chamfer_bwd are queued back to back on the stream; the nearest-neighbour indices stay in the scratch unless
 * idx_x (N,B) / idx_y (M,B) are given.  gx (D,N,B), gy (D,M,B) overwritten.  loss_host non-NULL => the stream is
 * synchronised.  ws: fx3d_chamfer_fwd_bwd_workspace_bytes. */
/* Capture: fx3d_chamfer_fwd_bwd: replayed -- with loss_host NULL. */
/* Batch axis: fx3d_chamfer_fwd_bwd_workspace_bytes: unbounded -- a host query.  fx3d_chamfer_fwd_bwd: B <= 536870911 -- as fx3d_nn1. */
FX3D_API fx3d_status fx3d_chamfer_fwd_bwd_workspace_bytes(int32_t N, int32_t M, int32_t B, int32_t D, size_t *bytes);
FX3D_API fx3d_status fx3d_chamfer_fwd_bwd(const float *x, int32_t N, const float *y, int32_t M, int32_t B, int32_t D,
                                          float w1, float w2, float gout, int64_t B_global, float *loss_dev,
                                          float *loss_host, float *gx, float *gy, int32_t *idx_x, int32_t *idx_y,
                                          void *ws, size_t ws_bytes, fx3d_stream_t s);

/* Adjoint of chamfer_distance(m_x::TriMesh, m_y::TriMesh, n) (src/metrics/mesh.jl:34-44: both meshes sampled, then
 * _chamfer_distance) w.r.t. the PADDED VERTICES of either mesh, for the forward's draws and nearest-neighbour indices, in one
 * call: fx3d_chamfer_bwd's gradient w.r.t. the sampled points (D = 3) goes onto the three vertices of every sampled face with
 * the barycentric weights of its draw (fx3d_sample_points_bwd).  x (3,N,B) / y (3,M,B): the samples;
 * face_idx_*, r1_*, r2_* (n,B): their draws (n = N resp. M); gverts_* (3,Vmax_*,B).  A side whose gverts is NULL is skipped (a
 * fitting loop differentiates w.r.t. the source mesh only).  accumulate = 0 overwrites gverts, else adds to it.
 * vf_rowptr_* / vf_ent_* (device copies of fx3d_build_vertex_faces' tables) select the ORDERED form for meshes it fits
 * (fx3d_sample_points_bwd_ordered(Fmax, n) for every requested side): no float atomics, every vertex's sum in the order of
 * fx3d_sample_points_bwd -- bit-reproducible; two launches (the rows and, by spare blocks, the gather's per-mesh tables into ws, then the
 * gather); ws: fx3d_chamfer_sampled_bwd_workspace_bytes.  NULL tables (or a mesh beyond the limits): ONE launch that scatters the rows
 * with global float atomics (sums in arrival order), ws unused -- ~9 us per call faster at one mesh of 5000 draws as a single call (inside
 * a fit iteration the ordered form is the faster one), slower at eight meshes, not reproducible. */
/* Capture: fx3d_chamfer_sampled_bwd, fx3d_chamfer_sampled_bwd_step: replayed. */
/* Batch axis: fx3d_chamfer_sampled_bwd_workspace_bytes: unbounded -- a host query.  fx3d_chamfer_sampled_bwd,
 * fx3d_chamfer_sampled_bwd_step, fx3d_chamfer_sampled_bwd_step_reg: B <= 536870911 -- as fx3d_nn1, and 2 B nsplit < 2^30. */
FX3D_API fx3d_status fx3d_chamfer_sampled_bwd_workspace_bytes(int32_t N, int32_t M, int32_t B, size_t *bytes);
FX3D_API fx3d_status fx3d_chamfer_sampled_bwd(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                                              const int32_t *idx_x, const int32_t *idx_y, float w1, float w2, float gout,
                                              int64_t B_global, const int32_t *faces_x, int32_t Vmax_x, int32_t Fmax_x,
                                              const int32_t *face_idx_x, const float *r1_x, const float *r2_x,
                                              float *gverts_x, const int32_t *faces_y, int32_t Vmax_y, int32_t Fmax_y,
                                              const int32_t *face_idx_y, const float *r1_y, const float *r2_y,
                                              float *gverts_y, int32_t accumulate, const int32_t *vf_rowptr_x,
                                              const int32_t *vf_ent_x, const int32_t *vf_rowptr_y, const int32_t *vf_ent_y,
                                              void *ws, size_t ws_bytes, fx3d_stream_t s);
/* The same for the source meshes alone (gradient w.r.t. mesh x only, ordered form required; B meshes of EQUAL vertex count V, so that
 * the optimiser's packed (3, B V) arrays are the padded (3, V, B) ones), with the optimiser step of the
 * fit_mesh loop (examples/fit_mesh.jl:87-88,108-110: Flux.Optimise.Momentum, then offset) applied by the thread that finishes a
 * vertex's gradient row g = gverts_x (accumulate: on top of the regularisers' gradient already in it):
 *   vel = rho vel - eta g;  params += vel;  out = base + params   (fx3d_momentum_step_offset's arithmetic), *ctr += inc.
 * The gather's launch does it: no launch of its own for the optimiser; gverts_x still receives g. */
FX3D_API fx3d_status fx3d_chamfer_sampled_bwd_step(const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                                                   const int32_t *idx_y, float w1, float w2, float gout,
                                                   const int32_t *faces_x, int32_t V, int32_t F, const int32_t *face_idx_x,
                                                   const float *r1_x, const float *r2_x, float *gverts_x, int32_t accumulate,
                                                   const int32_t *vf_rowptr_x, const int32_t *vf_ent_x, float rho, float eta,
                                                   float *vel, float *params, const float *base, float *out, uint64_t *ctr,
                                                   uint64_t inc, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- The fit iteration's regularisers as PASSENGERS of its sampling launches (round 6) ----------------------------------
 * examples/fit_mesh.jl:78-84: loss = chamfer_distance(m, tgt, 5000) + 0.1 laplacian_loss(m) + edge_loss(m).  The two regularisers
 * are launch-bound at tutorial scale (5 us kernels behind 4.4 us of graph-node latency each); handed over as an fx3d_mesh_reg their
 * forward runs as extra blocks of the DRAW launch (fx3d_sample_points_draw_pair_reg: loss_lap_dev, loss_edge_dev and the workspace's
 * unit rows are written; verts must be the vertices the draws' mesh 0 holds) and their adjoint as extra blocks of the launch that
 * forms the chamfer adjoint's rows (fx3d_chamfer_sampled_bwd_step_reg: gverts_x = accumulate ? gverts_x + g_reg : g_reg with
 * g_reg = fx3d_mesh_losses_bwd's bits for g_lap = w_lap gout, g_edge = w_edge gout, the sampling adjoint's gather then adds on top;
 * total_dev, optional, receives ((*base_dev or 0) + w_lap lap) + w_edge edge, fx3d_mesh_losses' sum).  Results are bit-identical to
 * fx3d_mesh_losses / fx3d_mesh_losses_bwd(reuse_forward = 1) / fx3d_chamfer_sampled_bwd_step(accumulate = 1) called one after the other:
 * two launches less per iteration.  All pointers are device pointers; V == B * Vmax of the source batch; ws:
 * fx3d_mesh_losses_workspace_bytes(V, E), the same for both calls. */
typedef struct fx3d_mesh_reg {
    const float *verts;          /* (3, V) packed vertices */
    int64_t V;
    const int32_t *rowptr, *colind;  /* the Laplacian's CSR, 0-based (fx3d_mesh_losses) */
    const float *vals;
    const int32_t *edges;        /* (E, 2) column-major: first vertices, then second vertices */
    int64_t E;
    float target, w_lap, w_edge;
    const float *base_dev;       /* the chamfer loss (optional) */
    float *loss_lap_dev, *loss_edge_dev;  /* required */
    float *total_dev;            /* optional */
    void *ws;
    size_t ws_bytes;
} fx3d_mesh_reg;
/* Capture: fx3d_sample_points_draw_pair_reg, fx3d_chamfer_sampled_bwd_step_reg: replayed -- the fx3d_mesh_reg structure is read
 * while recording. */
/* Batch axis: fx3d_sample_points_draw_pair_reg: unbounded -- B0 and B1 as fx3d_sample_points_draw. */
FX3D_API fx3d_status fx3d_sample_points_draw_pair_reg(const float *verts0, int32_t Vmax0, const int32_t *faces0, int32_t Fmax0,
                                                      const int32_t *faces_len0, int32_t B0, int32_t n0, uint64_t seed0, const void *cdf_ws0,
                                                      size_t ws_bytes0, float *out0, int32_t *face_out0, float *r1_out0, float *r2_out0,
                                                      const float *verts1, int32_t Vmax1, const int32_t *faces1, int32_t Fmax1,
                                                      const int32_t *faces_len1, int32_t B1, int32_t n1, uint64_t seed1, const void *cdf_ws1,
                                                      size_t ws_bytes1, float *out1, int32_t *face_out1, float *r1_out1, float *r2_out1,
                                                      const uint64_t *seed_dev, const fx3d_mesh_reg *reg, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_chamfer_sampled_bwd_step_reg(const float *x, int32_t N, const float *y, int32_t M, int32_t B, const int32_t *idx_x,
                                                       const int32_t *idx_y, float w1, float w2, float gout,
                                                       const int32_t *faces_x, int32_t V, int32_t F, const int32_t *face_idx_x,
                                                       const float *r1_x, const float *r2_x, float *gverts_x, int32_t accumulate,
                                                       const int32_t *vf_rowptr_x, const int32_t *vf_ent_x, float rho, float eta,
                                                       float *vel, float *params, const float *base, float *out, uint64_t *ctr,
                                                       uint64_t inc, void *ws, size_t ws_bytes, const fx3d_mesh_reg *reg, fx3d_stream_t s);

/* ---- k-NN graph (src/models/dgcnn.jl:3-7,36) ---------------------------------------------------
 * knn(KDTree(y), x, k+drop_first, true)[1][1+drop_first:end] for every point of every batch
 * element: idx:(k,N,B) int32 0-based sorted by (distance, index); dist:(k,N,B) squared distances
 * (optional).  y may equal x (self graph; drop_first=1 drops the rank-0 hit as the reference
 * does).  Any k+drop_first <= M and any D: the matrix-core kernels take k+drop_first <= 32 with M >= 64 (D = 3 and
 * 4 <= D <= 128) and, at D = 3, k+drop_first <= 64 with M >= 128 (fx3d_knn_ws also takes 4 <= D <= 128 up to k+drop_first = 128
 * there: candidate slices, see below); wave-per-query kernels k+drop_first <= 64 (D up to ~110),
 * a general selection kernel everything else
 * (k+drop_first up to M, any D) for M <= 36864 candidates; beyond that FX3D_ERR_UNSUPPORTED.
 * Order = Julia's isless on the Float32 squared distance, then the lower index: NaN distances (non-finite coordinates)
 * sort after +Inf, so every returned index is valid; fx3d_nn1 / the chamfer entry points use the same order.  The distance is
 * the Float32 one AS ROUNDED: where the squares underflow (a cloud of extent 1e-20: subnormal distances of a few bits; 1e-29:
 * every distance +0) the ties this makes are ordered by index, like those of +Inf distances at the other end. */
/* Capture: fx3d_knn, fx3d_knn_ws: replayed. */
/* Batch axis: fx3d_knn, fx3d_knn_workspace_bytes, fx3d_knn_ws: unbounded -- on the matrix-core routes (D = 3 with M >= 64 and
 * k + drop_first <= 32, or <= 64 on larger clouds; 4 <= D <= 128 with M >= 64 and k + drop_first <= 32), which fold the batch,
 * padded to a multiple of 8, into the grid's x, the pre-pass of fx3d_knn_ws included.  Every other shape takes a kernel with the
 * batch on the grid's y: B <= 65535 there, refused before any launch with a message that names B.  The candidate slices of
 * fx3d_knn_ws are planned only while B x slices <= 65535; beyond that the query returns the unsliced plan's size and the call
 * runs it, so query and call agree on both sides. */
FX3D_API fx3d_status fx3d_knn(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                              int32_t D, int32_t k, int32_t drop_first, int32_t *idx,
                              float *dist, fx3d_stream_t s);

/* The same search with caller-provided scratch.  In feature space (4 <= D <= 128 with D/4 a divisor of 256, 64 <= M <= 4096,
 * k+drop_first <= 32, 16-byte aligned clouds) the statistics and the fp16 image of every candidate cloud are then built once per
 * cloud by two small pre-pass launches instead of by every block of the search kernel (C4': 78 -> see DESIGN.md 3.2).
 * Few clouds with many rows (the grid of the matrix-core kernels would not fill the chip, or M > 4096 in feature space): the
 * search runs on 2 / 4 / 8 contiguous slices of every candidate cloud as so many virtual clouds and one wave per query merges the
 * slices' lists from the scratch (B = 1, N = M = 8192, D = 64: 758 -> 109 us; option "knn_slices": 0 automatic, 1 never, 2 / 4 / 8
 * forced).  Results are identical to fx3d_knn.  fx3d_knn_workspace_bytes returns 0 for shapes that have no use for scratch (it is a
 * function of the shape, the device's CU count and the options alone); a NULL, short or misaligned (256 bytes) workspace makes
 * fx3d_knn_ws behave exactly like fx3d_knn. */
FX3D_API fx3d_status fx3d_knn_workspace_bytes(int32_t N, int32_t M, int32_t B, int32_t D, int32_t k, int32_t drop_first,
                                              size_t *bytes);
FX3D_API fx3d_status fx3d_knn_ws(const float *x, int32_t N, const float *y, int32_t M, int32_t B, int32_t D, int32_t k,
                                 int32_t drop_first, int32_t *idx, float *dist, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* X[:, idxs] gather -> (F,k,N,B)  (src/models/dgcnn.jl:6 `X[:, knn(...)]`, cat at :36). */
/* Capture: fx3d_knn_gather, fx3d_edge_features, fx3d_edge_features_bwd, fx3d_edgeconv_graph: replayed. */
/* Batch axis: fx3d_knn_gather, fx3d_edge_features, fx3d_edge_features_bwd, fx3d_edgeconv_graph: unbounded -- grid-stride kernels
 * over all elements.  Layout 1 of fx3d_edge_features has the cloud on the grid's y: B <= 65535 there, and so for
 * fx3d_edgeconv_graph at layout 1 wherever it is not the fused F = 3 kernel; fx3d_edgeconv_graph off the matrix-core routes is
 * bound as fx3d_knn.  Each is refused before any launch, the search of fx3d_edgeconv_graph included. */
FX3D_API fx3d_status fx3d_knn_gather(const float *x, int32_t N, int32_t B, int32_t F, int32_t k,
                                     const int32_t *idx, float *out, fx3d_stream_t s);

/* EdgeConv graph features (src/models/dgcnn.jl:36-51): cat(X, KNNGraph - X, dims=1) for x (F,N,B) and
 * idx (k,N,B) from fx3d_knn, without materialising the gathered (F,k,N,B) array or the k copies of X.
 * layout 0: out (2F,k,N,B), the array at :45;  layout 1: out (k*N, 2F, B), the array handed to the 1x1
 * convolution after PermutedDimsArray + reshape at :48-51. */
FX3D_API fx3d_status fx3d_edge_features(const float *x, int32_t N, int32_t B, int32_t F, int32_t k,
                                        const int32_t *idx, int32_t layout, float *out, fx3d_stream_t s);
/* Adjoint w.r.t. x.  The graph is @nograd in the reference (src/models/dgcnn.jl:9): neighbours are
 * constants, gx[f,i,b] = sum_r gout[f,r,i,b] - gout[F+f,r,i,b] (rank order).  Overwrites gx (F,N,B). */
FX3D_API fx3d_status fx3d_edge_features_bwd(const float *gout, int32_t N, int32_t B, int32_t F, int32_t k,
                                            int32_t layout, float *gx, fx3d_stream_t s);
/* Self-kNN (drop_first) + fx3d_edge_features in one call: EdgeConv's whole graph build.  idx (k,N,B) out.
 * F = 3 (the first EdgeConv, coordinates) runs as ONE kernel: the neighbour search's epilogue writes the features. */
FX3D_API fx3d_status fx3d_edgeconv_graph(const float *x, int32_t N, int32_t B, int32_t F, int32_t k,
                                         int32_t layout, int32_t *idx, float *out, fx3d_stream_t s);

/* ---- TriMesh kernels --------------------------------------------------------------------------
 * The kernels read faces/edges as int32, 0-based; the reference's 1-based UInt32 / Int64 arrays (src/rep/mesh.jl:87-89)
 * enter through fx3d_index_upload / fx3d_index_convert below (converted on the device, cached with the mesh).  verts_packed (3,sumV); faces_packed (3,sumF) global
 * ids; verts_padded (3,Vmax,B) zero padded; faces_padded (3,Fmax,B) mesh-local ids (pad entries
 * ignored); faces_len (B) int32 -- all device. */

/* The reference's index arrays as they are (src/rep/mesh.jl:70-98: `TriMesh{T,R}` with R in {UInt32, Int64}, 1-based;
 * faces_packed / faces_padded / edges_packed, :884-896) -> the library's device form, int32 0-based, converted ON THE
 * DEVICE (one small kernel): the host passes `m._faces_packed` untouched, once per mesh, and keeps the result with it.
 *   index_type   FX3D_IDX_I32 / FX3D_IDX_U32 / FX3D_IDX_I64 (element type of src)
 *   index_base   subtracted from every element (1 for the reference's arrays, 0 for 0-based ones)
 *   clamp_pad    1: elements below index_base (the 0 padding of faces_padded) become 0 instead of -1
 *   limit        > 0: converted values must lie in [0, limit) (pad entries excepted); violations are COUNTED in *bad_dev
 *                (a caller-zeroed device counter, REQUIRED with a limit) and stored as 0 -- a kernel never dereferences them.
 *                limit == 0: only the int32 range is checked (UInt32 / Int64 values beyond it count, when bad_dev is given)
 * fx3d_index_upload: src is HOST memory (count elements); staged through ws (fx3d_index_upload_workspace_bytes, device)
 * and converted there; blocking like fx3d_memcpy_h2d.  fx3d_index_convert: src is device memory. */
typedef enum { FX3D_IDX_I32 = 0, FX3D_IDX_U32 = 1, FX3D_IDX_I64 = 2 } fx3d_index_type;
/* Capture: fx3d_index_convert: replayed.  fx3d_index_upload: copies to the host -- the other way: it stages the caller's pageable
 * array through the workspace and waits for that copy. */
FX3D_API fx3d_status fx3d_index_convert(const void *src_dev, int32_t index_type, int32_t index_base, int64_t count,
                                        int32_t clamp_pad, int64_t limit, int32_t *dst_dev, uint32_t *bad_dev,
                                        fx3d_stream_t s);
FX3D_API fx3d_status fx3d_index_upload_workspace_bytes(int32_t index_type, int64_t count, size_t *bytes);
FX3D_API fx3d_status fx3d_index_upload(const void *src_host, int32_t index_type, int32_t index_base, int64_t count,
                                       int32_t clamp_pad, int64_t limit, int32_t *dst_dev, uint32_t *bad_dev,
                                       void *ws, size_t ws_bytes, fx3d_stream_t s);

/* compute_faces_areas_packed (src/rep/mesh.jl:765-780): areas (sumF). */
/* Capture: fx3d_faces_areas_packed, fx3d_faces_areas_padded: replayed. */
FX3D_API fx3d_status fx3d_faces_areas_packed(const float *verts, int64_t V, const int32_t *faces,
                                             int64_t F, float *areas, fx3d_stream_t s);
/* compute_faces_areas_padded (src/rep/mesh.jl:799-808): areas (1,Fmax,B), zero padded. */
/* Batch axis: fx3d_faces_areas_padded: unbounded -- a grid-stride kernel over B * Fmax faces. */
FX3D_API fx3d_status fx3d_faces_areas_padded(const float *verts_padded, int32_t Vmax,
                                             const int32_t *faces_padded, int32_t Fmax,
                                             const int32_t *faces_len, int32_t B, float *areas,
                                             fx3d_stream_t s);

/* ---- vertex and face normals (src/rep/mesh.jl:589-621, 689-699) and their adjoints w.r.t. verts_packed ----------------
 * verts (3,V) packed, faces (3,F) packed global 0-based ids (V = sum V_i, F = sum F_i).  vf_rowptr (V+1) / vf_ent (3F): device
 * copies of fx3d_build_vertex_faces' tables of the PACKED faces (B = 1, Vmax = V, Fmax = F): entries face * 4 + corner,
 * ascending per vertex.  c_r(f) = _lg_cross(p[r+1] - p[r], p[r+2] - p[r]) over face f's corners p[0..2], taken cyclically
 * (r = 0: the operand order of the face areas).  All arithmetic is unfused Float32.
 * Definition (what the reference computes on the CPU, not what its docstring says): each of the three statements
 * `vertex_normals[:, faces[r, :]] += c_r` lowers to `A[:, I] = A[:, I] + X`, which is LAST WRITE WINS when I repeats a vertex.
 * So the raw normal of vertex v is ((+0 + c_0(w_0)) + c_1(w_1)) + c_2(w_2), where w_r is the highest-numbered face whose
 * corner r is v and a term is skipped when v is never corner r -- not a sum over all adjacent faces.  It then goes through
 * _normalize (src/rep/utils.jl:23-29): n = raw ./ max(s, 1f-6), s = sqrt((x*x + y*y) + z*z), where Julia's max returns NaN for
 * a NaN s.  Vertices in no face and degenerate faces give 0; -0 components become +0 for vertex normals (the +0 start) and stay
 * -0 for face normals, which are _normalize(c_0(f)).  Results are the same bits on every run and for every launch grid.
 * Adjoints: the exact derivative of the forward AS COMPUTED (the winners are fixed by the topology).  Per normal (vertex, or
 * face), g_raw = (g - n * ((n.x*g.x + n.y*g.y) + n.z*g.z)) / s  (component-wise: g.x - (n.x * dot), then / s)  when s > 1f-6,
 * otherwise (eps is the max, or s is NaN) g / 1f-6.  Then vertex u walks its table entries (f, t) in ascending order and, for
 * r = 0, 1, 2 whose role counts -- (f, r) is its owner's winner (vertex normals), r = 0 (face normals) -- adds corner t's term
 * of c_r(f)'s Jacobian transpose at g_raw of the role's owner (vertex faces[r, f] / face f): with a = p[r+1] - p[r],
 * b = p[r+2] - p[r], corner r+1 gets cross(b, g), corner r+2 gets cross(g, a), corner r -(cross(b, g) + cross(g, a)),
 * component by component.  The sum starts from gverts[u] (accumulate != 0) or +0, one term at a time: acc.x = acc.x + term.x.
 * This is not a claim about what Zygote returns through the reference's Buffer when corner rows repeat.
 * No float atomics, no memset, no host synchronisation: every launch can be captured into a graph.
 *
 * fx3d_verts_normals_packed: normals (3,V).  winner_mask (3,F) bytes, optional (NULL: not written): byte 3 f + r is 1 when
 *   (f, r) is the winner of vertex faces[r, f], else 0 -- every byte is written.  It depends on the topology only.
 * fx3d_verts_normals_bwd: gout (3,V) -> gverts (3,V); winner_mask from fx3d_verts_normals_packed on the same faces.
 * fx3d_faces_normals_packed (src/rep/mesh.jl:689-699): normals (3,F).  One launch, face-parallel.
 * fx3d_faces_normals_bwd: gout (3,F) -> gverts (3,V).
 * The adjoints are two launches each (g_raw into ws, then the gather): ws of fx3d_normals_workspace_bytes(V, F), device.
 * padded / list forms (:640-670, :719-746): fx3d_packed_to_padded of the packed result with verts_len / faces_len.
 * V < 2^31, F < 2^29. */
FX3D_API fx3d_status fx3d_normals_workspace_bytes(int64_t V, int64_t F, size_t *bytes);
/* Capture: fx3d_verts_normals_packed, fx3d_verts_normals_bwd, fx3d_faces_normals_packed, fx3d_faces_normals_bwd: replayed. */
FX3D_API fx3d_status fx3d_verts_normals_packed(const float *verts, int64_t V, const int32_t *faces, int64_t F,
                                               const int32_t *vf_rowptr, const int32_t *vf_ent, float *normals,
                                               uint8_t *winner_mask, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_verts_normals_bwd(const float *verts, int64_t V, const int32_t *faces, int64_t F,
                                            const int32_t *vf_rowptr, const int32_t *vf_ent, const uint8_t *winner_mask,
                                            const float *gout, float *gverts, int32_t accumulate, void *ws, size_t ws_bytes,
                                            fx3d_stream_t s);
FX3D_API fx3d_status fx3d_faces_normals_packed(const float *verts, int64_t V, const int32_t *faces, int64_t F,
                                               float *normals, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_faces_normals_bwd(const float *verts, int64_t V, const int32_t *faces, int64_t F,
                                            const int32_t *vf_rowptr, const int32_t *vf_ent, const float *gout, float *gverts,
                                            int32_t accumulate, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* _sample_points + _rand_barycentric_coords (src/transforms/mesh_func.jl:60-82) with the random
 * draws supplied: face_idx (n,B) int32 mesh-local 0-based, r1,r2 (n,B) in [0,1).  out (3,n,B). */
/* Capture: fx3d_sample_points_explicit, fx3d_sample_points, fx3d_sample_points_cdf, fx3d_sample_points_draw,
 * fx3d_sample_points_cdf_pair, fx3d_sample_points_draw_pair: replayed -- the seed is frozen; *seed_dev, read on the device when the
 * graph runs, is what moves it from one replay to the next. */
/* Batch axis: fx3d_sample_points_explicit, fx3d_sample_points_workspace_bytes, fx3d_sample_points, fx3d_sample_points_cdf,
 * fx3d_sample_points_draw, fx3d_sample_points_cdf_pair, fx3d_sample_points_draw_pair: unbounded -- one block per mesh on the
 * grid's x (the CDF) and grid-stride kernels over B * n samples (the draws).  Beyond 32768 faces per mesh (or the option cdf_multiblock_from) the CDF is built by
 * several blocks per mesh with the meshes on the grid's y: B <= 65535 there, refused by the argument check (of a pair: for both
 * batches before either is launched). */
FX3D_API fx3d_status fx3d_sample_points_explicit(const float *verts_padded, int32_t Vmax,
                                                 const int32_t *faces_padded, int32_t Fmax,
                                                 int32_t B, int32_t n, const int32_t *face_idx,
                                                 const float *r1, const float *r2, float *out,
                                                 fx3d_stream_t s);

FX3D_API fx3d_status fx3d_sample_points_workspace_bytes(int32_t Fmax, int32_t B, size_t *bytes);

/* sample_points(m, n; eps) (src/transforms/mesh_func.jl:21-58), drawing on device:
 * face ~ Categorical(area/ max(sum area, eps)) through a Float64 CDF (the reference computes the
 * probabilities in Float64 too, :32-39, including the last-padded-column fix-up), Philox4x32-10
 * counter RNG keyed by `seed`.  out (3,n,B); face_out, r1_out, r2_out (n,B) optional: the draws,
 * so that the adjoint (fx3d_sample_points_bwd) can be taken for the same sample. */
FX3D_API fx3d_status fx3d_sample_points(const float *verts_padded, int32_t Vmax,
                                        const int32_t *faces_padded, int32_t Fmax,
                                        const int32_t *faces_len, int32_t B, int32_t n,
                                        double eps, uint64_t seed, float *out, int32_t *face_out,
                                        float *r1_out, float *r2_out, void *ws, size_t ws_bytes,
                                        fx3d_stream_t s);

/* The two halves of fx3d_sample_points.  The CDF (areas -> Float64 probabilities -> prefix sums, :27-39) depends
 * only on the mesh: a caller keeps it while the vertices do not change (the target mesh of a fitting loop).  The
 * draw (:41-58) uses seed + *seed_dev (seed_dev optional, device memory): a captured graph replays with fresh
 * samples when fx3d_counter_add advances the device part.  The CDF is summed in a fixed radix-32 tree order (bit-identical to
 * oracle/flux3d_oracle.c): one launch for meshes of up to 32 768 faces, five (all blocks of the chip) beyond, Fmax <= 33 554 432. */
FX3D_API fx3d_status fx3d_sample_points_cdf(const float *verts_padded, int32_t Vmax,
                                            const int32_t *faces_padded, int32_t Fmax,
                                            const int32_t *faces_len, int32_t B, double eps, void *ws,
                                            size_t ws_bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_sample_points_draw(const float *verts_padded, int32_t Vmax,
                                             const int32_t *faces_padded, int32_t Fmax,
                                             const int32_t *faces_len, int32_t B, int32_t n, uint64_t seed,
                                             const uint64_t *seed_dev, const void *cdf_ws, size_t ws_bytes,
                                             float *out, int32_t *face_out, float *r1_out, float *r2_out,
                                             fx3d_stream_t s);

/* Both meshes of chamfer_distance(m1::TriMesh, m2::TriMesh, n) (src/metrics/mesh.jl:41-42) in ONE launch per half: the two
 * CDF builds (when both batches take the same one-block kernel variant; otherwise one after the other) and the two draws.
 * Bit-identical to two separate fx3d_sample_points_cdf / fx3d_sample_points_draw calls; saves two launch-bound kernels per
 * evaluation (C3: 66 -> 57 us).  seed_dev (optional) is added to both seeds. */
FX3D_API fx3d_status fx3d_sample_points_cdf_pair(const float *verts0, int32_t Vmax0, const int32_t *faces0, int32_t Fmax0,
                                                 const int32_t *faces_len0, int32_t B0, void *ws0, size_t ws_bytes0,
                                                 const float *verts1, int32_t Vmax1, const int32_t *faces1, int32_t Fmax1,
                                                 const int32_t *faces_len1, int32_t B1, void *ws1, size_t ws_bytes1,
                                                 double eps, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_sample_points_draw_pair(const float *verts0, int32_t Vmax0, const int32_t *faces0, int32_t Fmax0,
                                                  const int32_t *faces_len0, int32_t B0, int32_t n0, uint64_t seed0,
                                                  const void *cdf_ws0, size_t ws_bytes0, float *out0, int32_t *face_out0,
                                                  float *r1_out0, float *r2_out0, const float *verts1, int32_t Vmax1,
                                                  const int32_t *faces1, int32_t Fmax1, const int32_t *faces_len1, int32_t B1,
                                                  int32_t n1, uint64_t seed1, const void *cdf_ws1, size_t ws_bytes1,
                                                  float *out1, int32_t *face_out1, float *r1_out1, float *r2_out1,
                                                  const uint64_t *seed_dev, fx3d_stream_t s);

/* Adjoint of sample_points w.r.t. verts_padded for the same draws (Zygote through :67-71):
 * gverts_padded (3,Vmax,B) = sum of w_k * gout over the draws that hit each vertex.  accumulate = 0 overwrites gverts;
 * accumulate != 0 adds to it (this and the two mesh-loss adjoints then sum into one gradient buffer: the fit_mesh
 * objective's three terms without separate buffers, memsets and a final sum).
 * ORDERED form (vf_rowptr (Vmax+1,B) / vf_ent (3 Fmax,B): device copies of fx3d_build_vertex_faces' tables; meshes whose draws
 * and tables fit one CU's LDS -- 4 Fmax + 22.25 n + 18 K bytes <= 156 KB, i.e. up to ~5300 draws at 5120 faces (the reference's default is
 * 5000); fx3d_sample_points_bwd_ordered answers for a shape): g[v] = base[v] + sum over the (face, corner) pairs holding v,
 * ascending, of (0 + sum over the face's draws k, ascending, of w_corner(k) * gout[k]) in unfused Float32 -- no float atomics, the
 * same bits on every run (one block per mesh: draws bucketed by face and staged in LDS).
 * NULL tables, or a mesh beyond those limits: scatter with global float atomics (sums in arrival order). */
/* Batch axis: fx3d_build_vertex_faces: unbounded -- a host loop over the meshes. */
FX3D_API fx3d_status fx3d_build_vertex_faces(const int32_t *faces_padded_host, const int32_t *faces_len_host, int32_t Vmax,
                                             int32_t Fmax, int32_t B, int32_t *vf_rowptr_host, int32_t *vf_ent_host);
FX3D_API fx3d_status fx3d_sample_points_bwd_ordered(int32_t Fmax, int32_t n, int32_t *ordered);
/* Capture: fx3d_sample_points_bwd: replayed. */
/* Batch axis: fx3d_sample_points_bwd: B <= 67108863 -- 16 B < 2^30 (the ordered form's grid); the batch lies on the grid's x. */
FX3D_API fx3d_status fx3d_sample_points_bwd(const int32_t *faces_padded, int32_t Vmax,
                                            int32_t Fmax, int32_t B, int32_t n,
                                            const int32_t *face_idx, const float *r1,
                                            const float *r2, const float *gout, float *gverts,
                                            int32_t accumulate, const int32_t *vf_rowptr, const int32_t *vf_ent,
                                            fx3d_stream_t s);

/* out[i] = a*x[i] + b*y[i] (+ c*z[i] when z != NULL), Float32, unfused.  The device-side arithmetic of
 * the fit_mesh loop: offset!(m, delta) is verts + delta (src/transforms/mesh_func.jl:409-416, a = b = 1),
 * the sum of the three loss gradients, and the Momentum update (examples/fit_mesh.jl:87-110). */
/* Capture: fx3d_lincomb, fx3d_momentum_step, fx3d_momentum_step_offset, fx3d_packed_to_padded, fx3d_padded_to_packed: replayed --
 * verts_len_host is read while recording. */
FX3D_API fx3d_status fx3d_lincomb(int64_t n, float a, const float *x, float b, const float *y, float c,
                                  const float *z, float *out, fx3d_stream_t s);
/* Flux.Optimise.Momentum(eta, rho) on device arrays (examples/fit_mesh.jl:87-88,110): v <- rho*v - eta*g, then
 * x <- x + v, in one pass with the arithmetic of the two fx3d_lincomb calls it replaces. */
FX3D_API fx3d_status fx3d_momentum_step(int64_t n, float rho, float eta, const float *g, float *v, float *x,
                                        fx3d_stream_t s);
/* The same update plus what the next iteration of the fit loop starts with, in one launch: out <- base + x (the offset mesh,
 * offset(src, x), src/transforms/mesh_func.jl:435-438, same unfused arithmetic as fx3d_lincomb(1, base, 1, x)) and, when ctr is
 * not NULL, *ctr += inc (the sampling seeds' device counter, fx3d_counter_add). */
FX3D_API fx3d_status fx3d_momentum_step_offset(int64_t n, float rho, float eta, const float *g, float *v, float *x,
                                               const float *base, float *out, uint64_t *ctr, uint64_t inc, fx3d_stream_t s);
/* _packed_to_padded / _padded_to_packed for (3,*) Float32 vertex arrays without leaving the device
 * (src/rep/utils.jl:119-181).  verts_len is a HOST array of B lengths. */
/* Batch axis: fx3d_packed_to_padded, fx3d_padded_to_packed: unbounded -- one device copy per mesh, no kernel. */
FX3D_API fx3d_status fx3d_packed_to_padded(const float *packed, const int64_t *verts_len_host, int32_t B,
                                           int32_t Vmax, float *padded, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_padded_to_packed(const float *padded, const int64_t *verts_len_host, int32_t B,
                                           int32_t Vmax, float *packed, fx3d_stream_t s);

/* Scratch for the two mesh losses (bytes), count = E or V. */
FX3D_API fx3d_status fx3d_mesh_loss_workspace_bytes(int64_t count, size_t *bytes);

/* edge_loss(m, target) (src/metrics/mesh.jl:24-32).  edges (E,2) int32 0-based packed vertex
 * ids, column-major (first E entries = column 1).  loss_dev device float; loss_host optional. */
/* Capture: fx3d_edge_loss, fx3d_edge_loss_bwd, fx3d_edge_loss_bwd_adj, fx3d_laplacian_loss, fx3d_laplacian_loss_bwd,
 * fx3d_laplacian_loss_bwd_sym, fx3d_mesh_losses, fx3d_mesh_losses_bwd: replayed -- the two losses with loss_host NULL. */
FX3D_API fx3d_status fx3d_edge_loss(const float *verts, int64_t V, const int32_t *edges,
                                    int64_t E, float target, float *loss_dev, float *loss_host,
                                    void *ws, size_t ws_bytes, fx3d_stream_t s);
/* d edge_loss / d verts * gout -> gverts (3,V) (added when accumulate != 0; Zygote through src/metrics/mesh.jl:27-31).
 * fx3d_edge_loss_bwd: SCATTER form for a caller that holds only an edge list (any list): float atomics (+ a memset when
 * accumulate == 0), the last bit depends on their arrival order.
 * fx3d_edge_loss_bwd_adj: GATHER form over the vertex adjacency in CSR (rowptr (V+1), colind: neighbours ascending; a
 * diagonal entry is skipped, so the Laplacian's rowptr / colind of the same edge list serve as they are,
 * src/rep/mesh.jl:957-1002): vertex i adds its edges' terms in the order in which the reference's edge-by-edge
 * accumulation over the sorted edge list reaches it -- one launch, no float atomics, no memset, bit-identical run to run
 * and to the CPU restatement.  E = number of edges (the mean's denominator).  The wrappers use this one. */
FX3D_API fx3d_status fx3d_edge_loss_bwd(const float *verts, int64_t V, const int32_t *edges,
                                        int64_t E, float target, float gout, float *gverts,
                                        int32_t accumulate, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_edge_loss_bwd_adj(const float *verts, int64_t V, const int32_t *rowptr,
                                            const int32_t *colind, int64_t E, float target, float gout,
                                            float *gverts, int32_t accumulate, fx3d_stream_t s);

/* laplacian_loss(m) (src/metrics/mesh.jl:9-15) with L in CSR (rows = vertices, columns
 * ascending, values Float32 as built by _compute_laplacian_packed, src/rep/mesh.jl:957-1002). */
FX3D_API fx3d_status fx3d_laplacian_loss(const float *verts, int64_t V, const int32_t *rowptr,
                                         const int32_t *colind, const float *vals,
                                         float *loss_dev, float *loss_host, void *ws,
                                         size_t ws_bytes, fx3d_stream_t s);
/* d laplacian_loss / d verts * gout -> gverts (3,V) (added when accumulate != 0).
 * fx3d_laplacian_loss_bwd: ANY CSR (asymmetric, pruned, directed, duplicate columns): the row-by-row scatter with float
 * atomics (+ a memset when accumulate == 0) -- always the adjoint of fx3d_laplacian_loss; the last bit depends on the
 * atomics' arrival order.
 * fx3d_laplacian_loss_bwd_sym: gathered per vertex in the order of the reference's row-by-row accumulation: one launch,
 * no float atomics, bit-identical run to run and to the CPU restatement.  PRECONDITION: L structurally symmetric (i in
 * row r <=> r in row i: the Laplacian of an undirected edge list is, src/rep/mesh.jl:957-1002) without duplicate columns.
 * missing_dev (optional): a caller-zeroed device counter that receives the number of stored entries whose transpose is
 * absent -- non-zero means the precondition did not hold and those contributions are missing from gverts.  Option
 * "lap_bwd_scatter" = 1 routes this entry point to the scatter (A/B).  The wrappers use this one. */
FX3D_API fx3d_status fx3d_laplacian_loss_bwd(const float *verts, int64_t V, const int32_t *rowptr,
                                             const int32_t *colind, const float *vals, float gout,
                                             float *gverts, int32_t accumulate, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_laplacian_loss_bwd_sym(const float *verts, int64_t V, const int32_t *rowptr,
                                                 const int32_t *colind, const float *vals, float gout,
                                                 float *gverts, int32_t accumulate, uint32_t *missing_dev,
                                                 fx3d_stream_t s);

/* Both mesh losses in ONE launch and both adjoints in ONE gather launch -- the regularisers of the fit_mesh objective
 * (examples/fit_mesh.jl:80-83), launch bound at teapot scale.  rowptr/colind/vals: the Laplacian CSR of the SAME edge
 * list `edges` (E,2) (both are per-mesh caches of the reference, src/rep/mesh.jl:907-1002).
 * Forward: loss_lap_dev / loss_edge_dev (optional) receive laplacian_loss(m) / edge_loss(m, target); total_dev (optional)
 * receives ((*base_dev or 0) + w_lap*lap) + w_edge*edge in Float32, unfused -- the tutorial's sum in its order.  The
 * workspace keeps the Laplacian's unit rows for the adjoint.
 * Adjoint: gverts (3,V) = g_lap * d laplacian_loss/dv + g_edge * d edge_loss/dv (added to gverts when accumulate != 0),
 * gathered per vertex in the order of the reference's row-by-row / edge-by-edge accumulation: no float atomics, results
 * bit-identical run to run and to the CPU restatement.  reuse_forward != 0: fx3d_mesh_losses ran on the same vertices
 * with the same workspace since they last changed (its unit rows are reused); 0: they are rebuilt first. */
FX3D_API fx3d_status fx3d_mesh_losses_workspace_bytes(int64_t V, int64_t E, size_t *bytes);
FX3D_API fx3d_status fx3d_mesh_losses(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind,
                                      const float *vals, const int32_t *edges, int64_t E, float target, float w_lap,
                                      float w_edge, const float *base_dev, float *loss_lap_dev, float *loss_edge_dev,
                                      float *total_dev, void *ws, size_t ws_bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_mesh_losses_bwd(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind,
                                          const float *vals, int64_t E, float target, float g_lap, float g_edge,
                                          int32_t reuse_forward, float *gverts, int32_t accumulate, void *ws,
                                          size_t ws_bytes, fx3d_stream_t s);

/* ---- pointcloud_to_voxel (src/conversions.jl:91-131) ------------------------------------------------
 * points (3,N,B) -> voxels (res,res,res,B) Float32 0/1: voxel set iff the nearest cloud point of its
 * lattice centre lies within sqrt(0.6)/res after normalising the cloud by its scalar min/max; Float64
 * distance test exactly as at :125-129 (lattice (i+0.5)/res for i = 1..res, first array dimension = the
 * reference's innermost loop variable z).  ws: fx3d_voxel_workspace_bytes(B). */
/* Capture: fx3d_pointcloud_to_voxel: replayed. */
/* Batch axis: fx3d_voxel_workspace_bytes: unbounded -- a host query.  fx3d_pointcloud_to_voxel: B <= 65535 -- the scatter kernel
 * has the cloud on the grid's y; refused by the argument check, before `voxels` is cleared, with a message that names B. */
FX3D_API fx3d_status fx3d_voxel_workspace_bytes(int32_t B, size_t *bytes);
FX3D_API fx3d_status fx3d_pointcloud_to_voxel(const float *points, int32_t N, int32_t B, int32_t res,
                                              float *voxels, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- trimesh_to_voxel (src/conversions.jl:133-207) -------------------------------------------------
 * Padded meshes (the sampler's convention): verts_padded (3,Vmax,B) Float32, verts_len (B) int32 (every vertex counts,
 * also those no face uses), faces_padded (3,Fmax,B) int32 0-based mesh-local, faces_len (B) int32 -- all device.
 * voxels (res,res,res,B) Float32 0/1, overwritten: the x coordinate indexes the FIRST dimension (ix + res*(iy + res*iz)),
 * unlike fx3d_pointcloud_to_voxel.  Bit-identical to the reference's _voxelize (midpoint subdivision until every side^2
 * <= (1/res)^2, then trunc(p * (res-1))).  A mesh the reference cannot voxelise (zero extent, a NaN / Inf coordinate,
 * no vertices, a face id outside [0, verts_len)) is COUNTED in *bad_dev (optional, caller-zeroed device counter) and its
 * grid stays zero.  1 <= res <= 1024.  No host synchronisation (Capture: fx3d_trimesh_to_voxel: replayed).
 * ws: fx3d_trimesh_voxel_workspace_bytes(Vmax, Fmax, B, res). */
/* Batch axis: fx3d_trimesh_voxel_workspace_bytes: unbounded -- a host query.  fx3d_trimesh_to_voxel: B <= 65535 -- the counting
 * kernel has the mesh on the grid's y; refused by the argument check, before `voxels` is cleared, with a message that names B. */
FX3D_API fx3d_status fx3d_trimesh_voxel_workspace_bytes(int32_t Vmax, int32_t Fmax, int32_t B, int32_t res, size_t *bytes);
FX3D_API fx3d_status fx3d_trimesh_to_voxel(const float *verts_padded, int32_t Vmax, const int32_t *verts_len,
                                           const int32_t *faces_padded, int32_t Fmax, const int32_t *faces_len,
                                           int32_t B, int32_t res, float *voxels, uint32_t *bad_dev,
                                           void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- voxel_to_trimesh with algo :Exact (src/conversions.jl:209-232, 246-349) --------------------------
 * Two phases, because the output size depends on the data.  voxels (res,res,res,B) Float32 device, the first dimension
 * is x (the reference's CartesianIndices order).  1 <= res <= 1024.
 * fx3d_voxel_mesh_count: binarises `v >= thresh` (thresh is the reference's Float32(thresh)), clears interior cells
 *   (res >= 3: all six face neighbours set in the un-eroded grid, indices in 2:res-1) and counts the survivors.
 *   cubes_dev (B) int64: K of every grid.  bad_dev (B) uint32: elements outside [0, 1] or NaN per grid (the reference
 *   throws for a grid with any, and for K = 0).  Both are overwritten.  The workspace keeps what fx3d_voxel_mesh_emit needs.
 * fx3d_voxel_mesh_emit: consumes the workspace of the last fx3d_voxel_mesh_count with the same res and B (same stream).
 *   verts_packed (3, 8*sum K) Float32: grid after grid, cube after cube in column-major cell order, the reference's 8
 *   vertices of each cube divided by the grid's largest coordinate (a correctly rounded Float32 division).
 *   max_cubes: capacity of verts_packed in cubes (24 floats each); cubes beyond it are not written.
 *   faces_padded (3,Fmax,B) int32 0-based mesh-local, optional (NULL: none): cube j of a grid gets the reference's 12
 *   faces + 8j; entries behind a grid's 12 K faces are 0.  A grid with 12 K > Fmax gets no faces.  8 K must stay below
 *   2^31 (int32 face ids).  No entry point synchronises the host.  ws: fx3d_voxel_mesh_workspace_bytes(res, B). */
/* Capture: fx3d_voxel_mesh_count, fx3d_voxel_mesh_emit: replayed -- each in a graph of its own where the caller reads cubes_dev
 * between them. */
/* Batch axis: fx3d_voxel_mesh_workspace_bytes, fx3d_voxel_mesh_count, fx3d_voxel_mesh_emit: B <= 16777216 -- the batch lies on the
 * grid's x; 2^24 grids, and tiles per grid x B < 2^31. */
FX3D_API fx3d_status fx3d_voxel_mesh_workspace_bytes(int32_t res, int32_t B, size_t *bytes);
FX3D_API fx3d_status fx3d_voxel_mesh_count(const float *voxels, int32_t res, int32_t B, float thresh, int64_t *cubes_dev,
                                           uint32_t *bad_dev, void *ws, size_t ws_bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_voxel_mesh_emit(int32_t res, int32_t B, int64_t max_cubes, float *verts_packed,
                                          int32_t *faces_padded, int32_t Fmax, void *ws, size_t ws_bytes,
                                          fx3d_stream_t s);

/* The loss in the REFERENCE's own arithmetic, from the forward's NN indices: `mean((A .- B[:, nn]).^2) * 3.0f0` with
 * Base's Float32 pairwise sum (blocks of 1024, the materialised (D,N,B) array in column-major order;
 * src/metrics/pcloud.jl:47-50) -- bit for bit oracle/flux3d_oracle.c: fx3d_oracle_chamfer_loss_pairwise.  fx3d_chamfer_fwd
 * sums in Float64 (one rounding, order independent); this entry point is for a host that wants the reference's last bit.
 * Three small launches on `s`; loss_host optional (blocks).  ws: fx3d_chamfer_pairwise_workspace_bytes. */
/* Capture: fx3d_chamfer_loss_pairwise_f32: replayed -- with loss_host NULL. */
/* Batch axis: fx3d_chamfer_pairwise_workspace_bytes: unbounded -- a host query.  fx3d_chamfer_loss_pairwise_f32: B <= 536870911 --
 * as fx3d_nn1. */
FX3D_API fx3d_status fx3d_chamfer_pairwise_workspace_bytes(int32_t N, int32_t M, int32_t B, int32_t D, size_t *bytes);
FX3D_API fx3d_status fx3d_chamfer_loss_pairwise_f32(const float *x, int32_t N, const float *y, int32_t M, int32_t B,
                                                    int32_t D, const int32_t *idx_x, const int32_t *idx_y, float w1,
                                                    float w2, float *loss_dev, float *loss_host, void *ws,
                                                    size_t ws_bytes, fx3d_stream_t s);

/* ---- multi-GPU: one process per GPU, batch sharded contiguously -------------------
 * The reference is single-device; the only collective the sharded path needs is all-reduce(sum) of
 * the two Float64 chamfer partial sums (RCCL over xGMI).  librccl is loaded at run time.
 * Two ways to a communicator: fx3d_comm_bootstrap does the whole rendezvous itself (rank 0 creates the unique id and
 * hands it to the other ranks over TCP or a file: no torch, no MPI); or rank 0 calls fx3d_comm_unique_id, the host
 * moves the 128 bytes by any channel it has, and every rank calls fx3d_comm_init_rank.  Either way each rank makes its
 * own device current first (fx3d_set_device(local_rank)). */
FX3D_API fx3d_status fx3d_comm_unique_id(uint8_t *id128);
FX3D_API fx3d_status fx3d_comm_init_rank(fx3d_comm_t *comm, int32_t nranks, const uint8_t *id128,
                                         int32_t rank);
/* rendezvous: "tcp://host:port" (rank 0 listens on `port` -- loopback only when host is 127.0.0.1 / localhost --, the
 * others connect to host:port and retry until it is up; connections that do not speak the hand-shake {magic,
 * FX3D_COMM_TOKEN hash, nranks, rank} are dropped; nothing persists) or "file://path" (single node: rank 0 removes an
 * earlier job's leftovers, publishes {nonce, time, nranks, id} by rename of an O_EXCL | O_NOFOLLOW file, every reader
 * confirms the nonce and is acknowledged before it uses the id, rank 0 removes everything -- also when it gives up).
 * Under torchrun: tcp://$MASTER_ADDR:<a free port, e.g. $MASTER_PORT + 1>.  Blocks until all ranks have joined (120 s). */
FX3D_API fx3d_status fx3d_comm_bootstrap(fx3d_comm_t *comm, int32_t nranks, int32_t rank, const char *rendezvous);
/* The rendezvous alone: rank 0's 128 bytes arrive in every other rank's id128 (what fx3d_comm_bootstrap does between
 * fx3d_comm_unique_id and fx3d_comm_init_rank).  Host memory; needs neither a GPU nor RCCL. */
FX3D_API fx3d_status fx3d_comm_exchange_id(uint8_t *id128, int32_t nranks, int32_t rank, const char *rendezvous);
/* What the communicator says about itself (ncclCommCount / ncclCommUserRank) and the RCCL version code
 * (ncclGetVersion); any output may be NULL, comm may be NULL when only the version is asked for. */
FX3D_API fx3d_status fx3d_comm_info(fx3d_comm_t comm, int32_t *nranks, int32_t *rank, int32_t *rccl_version);
FX3D_API fx3d_status fx3d_comm_destroy(fx3d_comm_t comm);
/* Capture: fx3d_comm_allreduce_sum_f64, fx3d_comm_allreduce_max_f64, fx3d_chamfer_fwd_sharded, fx3d_chamfer_fwd_sharded_async:
 * collective -- an RCCL all-reduce inside a capture is not attempted. */
FX3D_API fx3d_status fx3d_comm_allreduce_sum_f64(fx3d_comm_t comm, double *buf_dev, int64_t count,
                                                 fx3d_stream_t s);
/* all-reduce(max): the control plane of a timing harness (max over ranks of an elapsed time; with any buffer: a barrier) */
FX3D_API fx3d_status fx3d_comm_allreduce_max_f64(fx3d_comm_t comm, double *buf_dev, int64_t count,
                                                 fx3d_stream_t s);
/* chamfer_distance of a batch sharded over the ranks of comm: kernel -> all-reduce(2 x f64) ->
 * finalise with B_global.  x:(D,N,B_local) y:(D,M,B_local) are THIS rank's slab (B_local may be 0);
 * sums_dev (2 doubles) and loss_dev device scratch/outputs; every rank receives the global loss. */
FX3D_API fx3d_status fx3d_chamfer_fwd_sharded(fx3d_comm_t comm, const float *x, int32_t N,
                                              const float *y, int32_t M, int32_t B_local, int32_t D,
                                              int64_t B_global, float w1, float w2, double *sums_dev,
                                              float *loss_dev, float *loss_host, void *ws,
                                              size_t ws_bytes, fx3d_stream_t s);

/* The same with the collective off the compute stream: kernel on `s`, all-reduce + finalise on `comm_stream` behind
 * the event `ready` (recorded on s), `done` (recorded on comm_stream) marks the loss.  No host wait: the next
 * evaluation's kernel on `s` overlaps this one's collective.  The caller rotates (sums_dev, loss_dev, ready, done) over
 * a few slots; the call itself makes `s` wait for the slot's previous `done` before the kernel overwrites sums_dev. */
FX3D_API fx3d_status fx3d_chamfer_fwd_sharded_async(fx3d_comm_t comm, const float *x, int32_t N, const float *y,
                                                    int32_t M, int32_t B_local, int32_t D, int64_t B_global,
                                                    float w1, float w2, double *sums_dev, float *loss_dev,
                                                    void *ws, size_t ws_bytes, fx3d_stream_t s,
                                                    fx3d_stream_t comm_stream, fx3d_event_t ready, fx3d_event_t done);

/* ---- host-pointer convenience variants --------------------------------------------------------------
 * The reference's CPU methods take plain `Array`s (src/metrics/pcloud.jl:54-70, src/models/dgcnn.jl:3-7,
 * src/transforms/mesh_func.jl:21-58, src/metrics/mesh.jl:9-32).  These take HOST buffers in Julia's column-major layout and
 * return host results: inputs are staged into device scratch owned by the calling thread (grow-only, reused), the SAME
 * device entry points run (there is no CPU code path), outputs are copied back, the call synchronises.  Convenient, not
 * fast: the PCIe copies are inside the call.  Indices 0-based int32 as everywhere at this boundary.
 * fx3d_chamfer_distance_host: any of loss / idx_x / idx_y may be NULL (not all).  fx3d_knn_host: y == NULL -> self
 * search (M ignored); dist optional.  Faces / edges / CSR as for the device entry points above. */
/* Batch axis: fx3d_chamfer_distance_host, fx3d_knn_host, fx3d_sample_points_host: unbounded -- host loops, no device. */
FX3D_API fx3d_status fx3d_chamfer_distance_host(const float *x, int32_t N, const float *y, int32_t M, int32_t B, int32_t D,
                                                float w1, float w2, float *loss, int32_t *idx_x, int32_t *idx_y);
FX3D_API fx3d_status fx3d_knn_host(const float *x, int32_t N, const float *y, int32_t M, int32_t B, int32_t D, int32_t k,
                                   int32_t drop_first, int32_t *idx, float *dist);
FX3D_API fx3d_status fx3d_sample_points_host(const float *verts_padded, int32_t Vmax, const int32_t *faces_padded,
                                             int32_t Fmax, const int32_t *faces_len, int32_t B, int32_t n, double eps,
                                             uint64_t seed, float *out);
FX3D_API fx3d_status fx3d_edge_loss_host(const float *verts, int64_t V, const int32_t *edges, int64_t E, float target,
                                         float *loss);
FX3D_API fx3d_status fx3d_laplacian_loss_host(const float *verts, int64_t V, const int32_t *rowptr, const int32_t *colind,
                                              const float *vals, float *loss);

/* ---- one process, several devices (SURVEY.md 8b "fx3d_comm_init_all(ndev)") ---------------------------------------
 * The reference is ONE Julia process (src/metrics/pcloud.jl:54-70): fx3d_comm_init_all gives such a host the
 * communicators of `ndev` of its devices (ncclCommInitAll; devices == NULL: 0..ndev-1) and, per device, a worker thread,
 * a stream and the scratch of a sharded evaluation.  fx3d_chamfer_fwd_multi: x[d] / y[d] are device d's slab
 * ((D,N,B_local[d]) / (D,M,B_local[d]) in ITS memory -- fx3d_set_device(d) + fx3d_malloc --, ignored where
 * B_local[d] == 0); every worker runs kernel -> all-reduce(sum) of 2 Float64 -> finalise with B_global on its stream; the
 * call returns when all of it is enqueued.  loss_host (optional): the global loss, read back from the first device
 * (blocks until it is there); losses_dev (optional, one device pointer per device, entries may be NULL): where each
 * device keeps its copy, valid after fx3d_multi_sync.  Calls on one handle must not overlap (one caller thread). */
FX3D_API fx3d_status fx3d_comm_init_all(fx3d_multi_t *multi, int32_t ndev, const int32_t *devices);
FX3D_API fx3d_status fx3d_multi_destroy(fx3d_multi_t multi);
FX3D_API fx3d_status fx3d_multi_info(fx3d_multi_t multi, int32_t *ndev, int32_t *devices, int32_t *rccl_version);
FX3D_API fx3d_status fx3d_multi_sync(fx3d_multi_t multi);
FX3D_API fx3d_status fx3d_chamfer_fwd_multi(fx3d_multi_t multi, const float *const *x, int32_t N,
                                            const float *const *y, int32_t M, const int32_t *B_local, int32_t D,
                                            int64_t B_global, float w1, float w2, float *loss_host,
                                            float *const *losses_dev);

/* ---- host-side topology (integer work; the reference keeps faces/edges/Laplacian on the host,
 *      src/rep/mesh.jl:87-97, and caches them forever) ------------------------------------------
 * _compute_edges_packed (src/rep/mesh.jl:907-955).  faces (3,F) host int64, `index_base` 0 or 1.
 * edges_out capacity 3F rows, column-major with leading dimension 3F?  No: written densely as
 * (E,2) column-major once E is known.  faces_to_edges (F,3) column-major, optional.
 * Outputs keep the caller's index_base. */
FX3D_API fx3d_status fx3d_build_edges_packed(const int64_t *faces, int64_t F, int64_t V,
                                             int32_t index_base, int64_t *edges_out,
                                             int64_t *faces_to_edges, int64_t *E_out);
/* _compute_laplacian_packed (src/rep/mesh.jl:957-1002) as 0-based CSR; capacity 2E+V. */
FX3D_API fx3d_status fx3d_build_laplacian_csr(const int64_t *edges, int64_t E, int64_t V,
                                              int32_t index_base, int32_t *rowptr,
                                              int32_t *colind, float *vals, int64_t *nnz_out);

/* ---- topology on the device: the same tables from device faces, for meshes that are born there -------------------
 * Every output is bit for bit what the host builders above (and fx3d_build_vertex_faces) write from the same faces.  All
 * arrays are device memory, int32 0-based.  Ordering is a stable radix sort: integer atomics only count bad ids, no output
 * bit depends on the order in which anything lands, no float atomics.  Ids outside their range are COUNTED in *bad_dev
 * (overwritten, one uint32) and stand in as vertex 0: a kernel never dereferences them; what such a call writes is defined
 * but meaningless.  No entry point synchronises the host.
 * Limits (an error status, like F = 0 or V = 0): 3F < 2^31; 2E + V < 2^31; Fmax < 2^29, 3 Fmax B < 2^31 and Vmax B < 2^31 - 1.
 *
 * _compute_edges_packed (src/rep/mesh.jl:907-955) in two phases, because E depends on the data.
 * fx3d_edges_dev_count: faces_packed (3,F), V = sum V_i.  *E_dev (int64): the number of distinct undirected edges -- the
 *   caller reads it back (the one synchronisation of a build) to size `edges`.  *bad_dev: corner ids outside [0, V)
 *   (REQUIRED).  The workspace keeps what fx3d_edges_dev_emit needs.
 * fx3d_edges_dev_emit: consumes the workspace of the last fx3d_edges_dev_count with the same F and V (same stream).
 *   edges (E,2) column-major: every (lo, hi), lo <= hi, ascending by (lo, hi); rows beyond the counted E are not written.
 *   faces_to_edges (F,3) column-major, optional (NULL: none; faces_packed is read only for it): edge ids in the reference's
 *   column order (e23, e31, e12) (:946).  ws: fx3d_edges_dev_workspace_bytes(F, V). */
FX3D_API fx3d_status fx3d_edges_dev_workspace_bytes(int64_t F, int64_t V, size_t *bytes);
/* Capture: fx3d_edges_dev_count, fx3d_edges_dev_emit, fx3d_laplacian_dev_csr, fx3d_vertex_faces_dev,
 * fx3d_faces_padded_to_packed_dev: replayed -- count and emit each in a graph of its own where the caller reads E_dev between them. */
FX3D_API fx3d_status fx3d_edges_dev_count(const int32_t *faces_packed, int64_t F, int64_t V, int64_t *E_dev,
                                          uint32_t *bad_dev, void *ws, size_t ws_bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_edges_dev_emit(const int32_t *faces_packed, int64_t F, int64_t V, int64_t E, int32_t *edges,
                                         int32_t *faces_to_edges, void *ws, size_t ws_bytes, fx3d_stream_t s);
/* _compute_laplacian_packed (src/rep/mesh.jl:957-1002) with the semantics of fx3d_build_laplacian_csr: edges (E,2)
 * column-major (any order), rowptr (V+1), colind / vals of capacity 2E + V (entries behind nnz are not written), *nnz_dev
 * (int64).  Columns ascend within a row, the diagonal is -1, off-diagonal values are deg > 0 ? (float)(1.0 / (double)deg) :
 * (float)deg where deg counts both ends of every edge (a self-edge adds 2); the copies of a repeated coordinate are summed in
 * the host's order, a self-edge's as (inv + inv) + (-1.0f): nnz = 2E + V - 2 (self-edges) for distinct edges.
 * bad_dev optional: edge ends outside [0, V).  ws: fx3d_laplacian_dev_workspace_bytes(E, V). */
FX3D_API fx3d_status fx3d_laplacian_dev_workspace_bytes(int64_t E, int64_t V, size_t *bytes);
FX3D_API fx3d_status fx3d_laplacian_dev_csr(const int32_t *edges, int64_t E, int64_t V, int32_t *rowptr, int32_t *colind,
                                            float *vals, int64_t *nnz_dev, uint32_t *bad_dev, void *ws, size_t ws_bytes,
                                            fx3d_stream_t s);
/* fx3d_build_vertex_faces for a padded batch on the device (the reference has no such table: it serves the ordered adjoint of
 * sample_points, src/rep/mesh.jl:67-71, and the vertex normals, :589-621): faces_padded (3,Fmax,B) mesh-local, faces_len (B; NULL: every
 * mesh has Fmax faces); vf_rowptr (Vmax+1,B), vf_ent (3 Fmax,B): the entries of a vertex are face * 4 + corner ascending, padding faces are ignored,
 * the slots of a column behind vf_rowptr[Vmax,b] are 0.  The packed table is the B = 1 call over faces_packed.  bad_dev
 * optional: ids outside [0, Vmax) in live faces and lengths outside [0, Fmax].  ws: fx3d_vertex_faces_dev_workspace_bytes. */
/* Batch axis: fx3d_vertex_faces_dev_workspace_bytes, fx3d_vertex_faces_dev: B <= 715827882 -- grid-stride kernels; 3 Fmax B and
 * Vmax B stay below 2^31. */
FX3D_API fx3d_status fx3d_vertex_faces_dev_workspace_bytes(int32_t Vmax, int32_t Fmax, int32_t B, size_t *bytes);
FX3D_API fx3d_status fx3d_vertex_faces_dev(const int32_t *faces_padded, const int32_t *faces_len, int32_t Vmax, int32_t Fmax,
                                           int32_t B, int32_t *vf_rowptr, int32_t *vf_ent, uint32_t *bad_dev, void *ws,
                                           size_t ws_bytes, fx3d_stream_t s);
/* _compute_faces_packed (src/rep/mesh.jl:884-896) from the padded device faces: faces_packed (3,sumF), mesh after mesh, each
 * id plus the vertex count of the meshes before it (nverts (B) int32).  sumF: capacity of faces_packed in faces (the sum of
 * faces_len); a mesh that would end behind it is not written.  ws: fx3d_faces_padded_to_packed_dev_workspace_bytes(B). */
/* Batch axis: fx3d_faces_padded_to_packed_dev_workspace_bytes, fx3d_faces_padded_to_packed_dev: unbounded -- one scanning block
 * and a grid-stride kernel. */
FX3D_API fx3d_status fx3d_faces_padded_to_packed_dev_workspace_bytes(int32_t B, size_t *bytes);
FX3D_API fx3d_status fx3d_faces_padded_to_packed_dev(const int32_t *faces_padded, const int32_t *faces_len,
                                                     const int32_t *nverts, int32_t Fmax, int32_t B, int64_t sumF,
                                                     int32_t *faces_packed, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- PointNet inference: (m::PointNet)(X) (src/models/pointnet.jl:62-85) in test mode -----------------------------
 * The forward (its gradients: "PointNet adjoint" below), Float32: BatchNorm uses its running statistics, Dropout is the identity.
 * x (3,N,B) device; point n of
 * cloud b has channels x[:,n,b].  PointNet(num_classes, 64): the reference's conv_block1 is fixed at 64 channels, so no
 * other K works there (src/models/pointnet.jl:41-60).  In the order the layers run (stnKD: :3-20, conv_bn_block:
 * src/models/utils.jl:1-3):
 *   stn   = stnKD(3):  conv 3->64, relu, BN . conv 64->128, relu, BN . conv 128->1024, relu, BN . max over the N points .
 *                      dense 1024->512, relu . dense 512->256, relu . BN(256) . dense 256->9;
 *                      T (3,3,B), T[i,j,b] = d[j + 3 i] (the reshape is column-major, then the transpose; no identity added)
 *   x'[j] = sum_i x[i] T[i,j,b] per point
 *   conv_block1:       conv 3->64, BN, relu (this order)                                   -> h (N,64,B)
 *   fstn  = stnKD(64): as stn with 64 input channels and a last dense 256->4096;  F (64,64,B), F[i,j,b] = d[j + 64 i]
 *   h'[j] = sum_i h[i] F[i,j,b] per point
 *   feat:              conv 64->128, relu, BN . conv 128->1024 (no activation), BN . max over N (= pooled (1024,B)) .
 *                      dense 1024->512, relu . BN(512) . dense 512->256, relu . (Dropout) . BN(256)
 *   cls:               dense 256->num_classes, relu (before the softmax, :58) = logits . softmax over the classes = probs
 * Arithmetic (the contract; tests/pointnet_ref.py restates it on the host):
 *   contraction (conv, dense, both transforms): acc = +0.0f; for c ascending: acc = fmaf(x[c], W[c,o], acc); conv and dense
 *     then add the bias with one Float32 addition and apply the activation (Flux: sigma.(W*x .+ b));
 *   relu = Julia's max(0, v): NaN stays NaN, relu(-0.0) = +0.0;
 *   BatchNorm, eps = 1f-5: (gamma * ((v - mu) / sqrt(var + eps))) + beta, every operation rounded to Float32, division
 *     and square root correctly rounded;
 *   max over the points = Julia's max (NaN wins, max(-0.0, +0.0) = +0.0): order-free;
 *   softmax: e = exp(z - max z), e / sum e with the sum in class order; exp is not pinned to a bit pattern.
 * logits, stn, fstn and pooled are bit-identical to that restatement and from run to run, whatever N, B and the launch
 * shape: one accumulator per output element, no contraction split over waves or blocks, no float atomics.
 * params_dev: ONE flat device Float32 buffer, the layers' arrays in forward order -- stn, conv_block1, fstn, feat, cls --,
 *   each layer as:  conv  W (Cin,Cout) column-major (Flux's (1,Cin,Cout)), then b (Cout);
 *                   BatchNorm  gamma, beta, mu, var (C each);
 *                   dense  W (out,in) column-major, then b (out).
 *   fx3d_pointnet_param_count(num_classes) is its length in floats.
 * probs (num_classes,B) is required; logits (num_classes,B), stn (3,3,B), fstn (64,64,B), pooled (1024,B) are optional
 * (NULL: not written).  Six launches on `s`, no host synchronisation, no host memory read after the argument check
 * (Capture: fx3d_pointnet_forward: replayed).  ws: fx3d_pointnet_workspace_bytes(N, B, num_classes), 16-byte aligned. */
FX3D_API fx3d_status fx3d_pointnet_param_count(int32_t num_classes, int64_t *count);
/* Batch axis: fx3d_pointnet_workspace_bytes, fx3d_pointnet_forward: B <= 65535 -- the point kernels have the cloud on the grid's y;
 * refused by the size check, the query included, with a message that names B. */
FX3D_API fx3d_status fx3d_pointnet_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_pointnet_forward(const float *params_dev, int32_t num_classes, const float *x, int32_t N,
                                           int32_t B, float *probs, float *logits, float *stn, float *fstn,
                                           float *pooled, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- DGCNN inference: (m::DGCNN)(X) (src/models/dgcnn.jl:113-147) in test mode ------------------------------------------
 * The forward (its gradients: "DGCNN adjoint" below), Float32: BatchNorm uses its running statistics, Dropout is the identity.  x (3,N,B) device.  DGCNN(num_classes,
 * K, npoints) with N == npoints: MaxPool((npoints,)) is then the maximum over all points of a cloud, which is what this
 * computes (for another N the reference's reshape to (1024,B) fails or mixes clouds; the host layers refuse it).
 * conv_bn_block / fc_bn_block (src/models/utils.jl:1-7) are conv or dense, BN, relu -- in this order.  In the order they run:
 *   EdgeConv1 = EdgeConv([3,32,64,64], K) (:32-71):  idx1 (K,N,B) = the K nearest neighbours of every point among its cloud's
 *                      points in coordinate space, the point itself (rank 0 of K+1) dropped: fx3d_knn's order and 0-based
 *                      indices; edge row (k,n) = [x_n (3), x_idx1(k,n) - x_n (3)]; conv 6->32, 32->64, 64->64, each BN, relu;
 *                      x1[c,n,b] = max over k                                             -> x1 (64,N,B)
 *   EdgeConv2 = EdgeConv([64,128,256], K):  the same on x1: idx2 from the 64-dimensional rows of x1; edge row of 128;
 *                      conv 128->128, 128->256, each BN, relu; max over k                 -> x2 (256,N,B)
 *   conv_3:            conv 256->1024, BN, relu; max over the N points                    -> pooled (1024,B)
 *   fc_4, fc_5:        dense 1024->512, BN, relu . dense 512->256, BN, relu . (Dropout)
 *   fc_6:              dense 256->num_classes = logits (no activation before the softmax, unlike PointNet) . softmax = probs
 * The reference's reshape(K, an N, B) / MaxPool((K,)) / reshape / permute (:57-68) is the maximum over k per (channel, point).
 * Arithmetic: the PointNet contract above, verbatim -- contraction as one fmaf chain from +0.0f over ALL 2F concatenated
 * channels ascending (the x_n half first), one Float32 bias addition, BatchNorm with eps = 1f-5 and every operation rounded
 * to Float32, relu and both maxima as Julia's max (NaN wins, max(-0.0, +0.0) = +0.0: order-free), the softmax as there.  The
 * edge difference is one Float32 subtraction.  (Flux's MaxPool is NNlib's; its NaN behaviour is not pinned here: Julia's max
 * is the definition.)  The (K N, 2F, B) edge array is never written to memory.
 * idx1, x1, idx2, x2, pooled and logits are bit-identical to the restatement tests/dgcnn_ref.py and from run to run, whatever
 * N, B, K and the launch shape: one accumulator per output element, no contraction split over waves or blocks, no float atomics.
 * params_dev: ONE flat device Float32 buffer in forward order -- EdgeConv1's three (conv, BN), EdgeConv2's two, conv_3's one,
 *   (fc_4 dense, BN), (fc_5 dense, BN), fc_6 -- each layer laid out as for PointNet (conv W (Cin,Cout) then b; BN gamma, beta,
 *   mu, var; dense W (out,in) then b).  fx3d_dgcnn_param_count(num_classes) is its length in floats.
 * 1 <= K <= N - 1, N <= 36864 (the neighbour search's general kernel), B <= 65535, N B K <= 2^31; anything else, a NULL
 * required pointer, a short workspace or one not 256-byte aligned is FX3D_ERR_INVALID_ARG before any launch.
 * probs (num_classes,B) is required; logits (num_classes,B), idx1 and idx2 (K,N,B) int32, x1 (64,N,B; 16-byte aligned),
 * x2 (256,N,B) and pooled (1024,B) are optional (NULL: not written).  Launches on `s` only (per EdgeConv what
 * fx3d_edgeconv_forward below launches -- the search through fx3d_knn_ws and the EdgeConv kernel --, then conv_3 and the
 * head), no host synchronisation, no host memory read after the argument check (Capture: fx3d_dgcnn_forward: replayed).
 * ws: fx3d_dgcnn_workspace_bytes(N, B, K, num_classes) -- x1, x2, per-tile maxima, the logits and one EdgeConv workspace (the
 * neighbour lists and the search's scratch), the larger of the two stages', which they use in turn. */
FX3D_API fx3d_status fx3d_dgcnn_param_count(int32_t num_classes, int64_t *count);
/* Batch axis: fx3d_dgcnn_workspace_bytes, fx3d_dgcnn_forward: B <= 65535 -- the EdgeConv and point kernels have the cloud on the
 * grid's y; refused by the size check, the query included, with a message that names B. */
FX3D_API fx3d_status fx3d_dgcnn_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_dgcnn_forward(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N,
                                        int32_t B, float *probs, float *logits, int32_t *idx1, float *x1, int32_t *idx2,
                                        float *x2, float *pooled, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- EdgeConv inference: (m::EdgeConv)(X) (src/models/dgcnn.jl:11-71) in test mode, for any layer widths -------------------
 * EdgeConv(layers, K) as a layer in its own right, Float32 (the gradient with respect to x: "EdgeConv input adjoint" below).  layers: a HOST array [F, c1, ..., cL] of nlayers
 * entries, the argument of the reference's constructor: L = nlayers - 1 conv_bn_blocks (src/models/utils.jl:1-3) 2F -> c1,
 * c1 -> c2, ..., each conv, BatchNorm with its running statistics, relu -- in this order.  x (F,N,B) device, out (cL,N,B):
 *   idx (K,N,B) = the K nearest neighbours of every point among its own cloud's F-dimensional rows, the point itself (rank 0 of
 *     K+1) dropped: fx3d_knn_ws(x, N, x, N, B, F, K, 1, ...) with its order and its 0-based indices;
 *   edge row (k,n) = [x_n (F), x_idx(k,n) - x_n (F)], the difference one Float32 subtraction; the L blocks on every row;
 *   out[c,n,b] = max over k.  The (K N, 2F, B) edge array is never written to memory.
 * idx_in == NULL: the search runs, and its lists are written to idx_out if that is given.  idx_in != NULL, (K,N,B) int32 on the
 * device: the search is skipped and these lists are used (static graphs, tests); idx_out is then not touched.  Defined
 * behaviour: an index outside [0, N) reads the point itself (an edge row [x_n, 0]).
 * Arithmetic: the PointNet / DGCNN contract above, verbatim -- one accumulator per output element, acc = fmaf(x[c], W[c,o], acc)
 * for c ascending from +0.0f over ALL 2F concatenated channels (the x_n half first), one Float32 bias addition, BatchNorm with
 * eps = 1f-5 and every operation rounded to Float32, relu and the maximum as Julia's max.  No contraction is split over waves
 * or blocks, no contraction is padded with zero channels, no float atomics: out and idx are bit-identical to the restatement
 * tests/edgeconv_ref.py and from run to run, whatever N, B, K and the launch shape, and EdgeConv([3,32,64,64], K) /
 * EdgeConv([64,128,256], K) on DGCNN's parameters give fx3d_dgcnn_forward's x1 / x2.
 * params_dev: ONE flat device Float32 buffer in forward order, per block conv W (Cin,Cout) column-major then b (Cout), then
 *   BatchNorm gamma, beta, mu, var (Cout each) -- the layout of the EdgeConv slices of the DGCNN buffer, so a slice of a DGCNN's
 *   parameters is a valid EdgeConv buffer.  fx3d_edgeconv_param_count(layers, nlayers) is its length in floats.
 * Envelope: 1 <= L <= 4, 1 <= F <= 128, every width in [1, 256] (no multiple of anything required) -- anything else is
 * FX3D_ERR_UNSUPPORTED; 1 <= K <= N - 1, N <= 36864 (the neighbour search), B <= 65535, N B K <= 2^31 -- anything else, a NULL
 * required pointer (params_dev, layers, x, out, ws), a short workspace or one not 256-byte aligned is FX3D_ERR_INVALID_ARG.
 * Every refusal comes before any device work and names the offending value in fx3d_last_error.
 * Launches on `s` only (the search through fx3d_knn_ws, one EdgeConv kernel), no host synchronisation, no host memory other
 * than `layers` read, and none after the argument check (Capture: fx3d_edgeconv_forward: replayed).  ws: fx3d_edgeconv_workspace_bytes(layers, nlayers,
 * K, N, B) -- the neighbour lists and the search's scratch. */
FX3D_API fx3d_status fx3d_edgeconv_param_count(const int32_t *layers, int32_t nlayers, int64_t *count);
/* Batch axis: fx3d_edgeconv_workspace_bytes, fx3d_edgeconv_forward: B <= 65535 -- the EdgeConv kernel has the cloud on the grid's
 * y; refused by the size check, the query included, with a message that names B. */
FX3D_API fx3d_status fx3d_edgeconv_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B,
                                                   size_t *bytes);
FX3D_API fx3d_status fx3d_edgeconv_forward(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K,
                                           const float *x, int32_t N, int32_t B, const int32_t *idx_in, float *out,
                                           int32_t *idx_out, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- EdgeConv input adjoint: the gradient of (m::EdgeConv)(X) with respect to X, test mode -----------------------------------
 * gx (F,N,B) = d sum(gout . out) / d x for out = fx3d_edgeconv_forward(x), in one fused kernel; the arguments up to B are the
 * forward's.  BatchNorm uses its running statistics.  The neighbours are constants: CreateSingleKNNGraph is @nograd
 * (src/models/dgcnn.jl:9), so gradient reaches x only through the repeated x_n of cat(X, KNNGraph - X), as fx3d_edge_features_bwd
 * states, and gx[:,n] depends on the K edge rows of point n alone.  No parameter gradients: the weights are constants here.
 * idx (K,N,B) and out (cL,N,B): the forward's lists and result.  idx == NULL: the search runs as in the forward (it is
 * deterministic: the lists are the forward's).  out == NULL: the forward runs first, into the workspace.  gout (cL,N,B).
 * With a_0[k,n,:] = [x_n, x_idx(k,n) - x_n] and a_l = relu(BN(conv_l(a_{l-1}))), the forward's bits, per cloud:
 *   maximum over k:  d_L[k,n,o] = gout[o,n] if out[o,n] > 0 and k is the smallest k with a_L[k,n,o] == out[o,n] (Float32
 *     comparison), else +0.  A NaN or non-positive out element passes nothing, and so does one that no k reproduces (defined
 *     behaviour for an out that did not come from this forward).
 *   per layer, l = L .. 1:  for l < L first d_l = (a_l > 0) ? d_l : +0;  dz_l = (d_l gamma_l) / sd_l, sd_l = sqrtf(var_l + 1f-5),
 *     both operations rounded to Float32;  d_{l-1}[k,n,c] = one fmaf chain from +0.0f over ALL o ascending,
 *     acc = fmaf(dz_l[k,n,o], W_l[c,o], acc).  The forward's contract, transposed: one accumulator per element, no contraction
 *     split over waves or blocks, none padded with zero channels, no term skipped because it is zero (0 * Inf is NaN).
 *   sum over k:  S[n,c] = sum_k d_0[k,n,c], Float32 additions from +0, k ascending, for the 2F channels;
 *   gx[f,n] = S[n,f] - S[n,F+f], one Float32 subtraction.
 * gx is bit-identical to the restatement tests/edgeconv_bwd_ref.py and from run to run, whatever N, B, K and the launch shape;
 * no float atomics, and no (K N, ., B) array in memory.
 * Deviation from the reference: NNlib's CPU max-pool adjoint is said to give the gradient to the first element that is
 * approximately the maximum, cuDNN gives it to an argmax; neither can be run here to settle it.  Here it goes to the first k
 * that EQUALS the maximum.  (Ties among positive maxima need two edge rows with the same last-layer value: repeated
 * neighbours, or hidden layers the relu has zeroed.)
 * Envelope, refusals, status codes and messages are fx3d_edgeconv_forward's: 1 <= L <= 4, 1 <= F <= 128, widths in [1, 256],
 * else FX3D_ERR_UNSUPPORTED; a bad K, N or B, a NULL required pointer (params_dev, layers, x, gout, gx, ws), a short workspace
 * or one not 256-byte aligned is FX3D_ERR_INVALID_ARG; each names the offending value and comes before any device work.  An
 * index outside [0, N) reads the point itself, as in the forward.
 * Launches on `s` only (the search and / or the forward where idx / out are NULL, one small kernel that lays the weights out
 * transposed in the workspace, the adjoint kernel), no host synchronisation, no host memory other than `layers` read, and none
 * after the argument check (Capture: fx3d_edgeconv_bwd: replayed).  ws: fx3d_edgeconv_bwd_workspace_bytes(layers, nlayers, K, N, B) -- the forward's
 * workspace, the lists, out and the transposed weights. */
/* Batch axis: fx3d_edgeconv_bwd_workspace_bytes, fx3d_edgeconv_bwd: B <= 65535 -- as fx3d_edgeconv_forward. */
FX3D_API fx3d_status fx3d_edgeconv_bwd_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B,
                                                       size_t *bytes);
FX3D_API fx3d_status fx3d_edgeconv_bwd(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x,
                                       int32_t N, int32_t B, const int32_t *idx, const float *out, const float *gout, float *gx,
                                       void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- EdgeConv parameter adjoint: the gradients of (m::EdgeConv)(X) with respect to its parameters, and to X, test mode --------
 * gparams = d sum(gout . out) / d params for out = fx3d_edgeconv_forward(x), a flat Float32 buffer with the layout of params_dev
 * (fx3d_edgeconv_param_count floats), and, if gx != NULL, gx (F,N,B) exactly as fx3d_edgeconv_bwd gives it, from one fused kernel
 * and two small finishing kernels.  BatchNorm in test mode: mu and var are constants (their slots are written as +0), gamma and
 * beta are parameters.  The neighbours are constants.  Arguments, idx == NULL and out == NULL as in "EdgeConv input adjoint".
 * Notation of "EdgeConv input adjoint"; for layer l = 1 .. L and every edge row (b, n, k):
 *   z_l = the forward's chain over c of a_{l-1}[c] W_l[c,o];  t_l = ((z_l + b_l) - mu_l) / sd_l;  a_l = relu(gamma_l t_l + beta_l).
 *   d_l, the gradient at the relu's argument, is what the input adjoint forms, bit for bit: d_L = gout at the first k that
 *   reproduces a positive out, else +0;  d_{l-1} = (a_{l-1} > 0) ? the chain over all o of dz_l Wt_l : +0;  dz_l = (d_l gamma_l) / sd_l.
 * Two sums over all edge rows per layer:
 *   H_l[c,o] = sum a_{l-1}[c] d_l[o]   (cin_l x cout_l)          h_l[o] = sum d_l[o]
 * and from them, every operation rounded to Float32, none dividing by gamma:
 *   dbeta_l[o]  = h_l[o]
 *   db_l[o]     = (h_l[o] gamma_l[o]) / sd_l[o]
 *   dW_l[c,o]   = (H_l[c,o] gamma_l[o]) / sd_l[o]
 *   dgamma_l[o] = (acc + (b_l[o] - mu_l[o]) h_l[o]) / sd_l[o],  acc = fmaf(W_l[c,o], H_l[c,o], acc) for c ascending from +0.0f
 *   (sum d z = sum_c W[c,o] H[c,o]: t_l is never kept).
 * The order of the sums is part of the contract.  It depends on (layers, K, N, B) alone -- not on the device, the launch shape,
 * how the kernel splits its work, the workspace or the run:
 *   a chunk is FX3D_EDGECONV_GRAD_CHUNK = 128 consecutive points of one cloud (the last chunk of a cloud may be shorter), made
 *   of tiles of 32 consecutive points.  Within a tile the points are visited in the order
 *     perm = 0,4, 1,5, 2,6, 3,7, 8,12, 9,13, 10,14, 11,15, 16,20, 17,21, 18,22, 19,23, 24,28, 25,29, 26,30, 27,31
 *   (pair r = 0 .. 15 is (q, q + 4) with q = (r mod 4) + 8 (r div 4)), points beyond the cloud's last one left out.
 *   H_l[c,o] of a chunk: ONE chain from +0.0f, acc = fmaf(a_{l-1}[row][c], d_l[row][o], acc), over the chunk's tiles ascending,
 *     within a tile k ascending, within a k the tile's points in the order perm.
 *   h_l[o] of a chunk: two chains of Float32 additions from +0 in the same order, one over the first points of the pairs
 *     (q), one over the second (q + 4), then first + second.
 *   H_l and h_l: one chain of Float32 additions from +0 over the chunk values, b ascending, within b the chunks ascending.
 *   (So a batch is not the sum of its clouds' separate results, and N > 128 is not one chain.)
 * gparams and gx are bit-identical to the restatement tests/edgeconv_pgrad_ref.py and from run to run; no float atomics, no
 * (K N, ., B) array in memory.  gx is fx3d_edgeconv_bwd's, bit for bit.
 * Envelope, refusals, their order, status codes and messages are fx3d_edgeconv_bwd's (required pointers: params_dev, layers, x,
 * gout, gparams, ws); every refusal comes before any device work.  Launches on `s` only (the search and / or the forward where
 * idx / out are NULL, the weight transpose, the kernel, two finishing kernels), no host synchronisation (Capture: fx3d_edgeconv_grad: replayed).
 * ws: fx3d_edgeconv_grad_workspace_bytes -- the input adjoint's, one partial of param_count floats per chunk and cloud, and the sums. */#define FX3D_EDGECONV_GRAD_CHUNK 128 /* points of one cloud whose rows are summed as one chain ("EdgeConv parameter adjoint") */
/* Batch axis: fx3d_edgeconv_grad_workspace_bytes, fx3d_edgeconv_grad: B <= 65535 -- as fx3d_edgeconv_forward. */
FX3D_API fx3d_status fx3d_edgeconv_grad_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B,
                                                        size_t *bytes);
FX3D_API fx3d_status fx3d_edgeconv_grad(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K, const float *x,
                                        int32_t N, int32_t B, const int32_t *idx, const float *out, const float *gout,
                                        float *gparams, float *gx, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- DGCNN adjoint: the gradients of (m::DGCNN)(X) with respect to its parameters and to X, test mode --------------------------
 * gparams = d sum(glogits . logits) / d params for logits = fx3d_dgcnn_forward(x), a flat Float32 buffer with the layout of
 * params_dev (fx3d_dgcnn_param_count floats), and, if gx != NULL, gx (3,N,B) = d sum(glogits . logits) / d x.  The arguments up
 * to B are the forward's.  glogits (num_classes,B) is the upstream gradient with respect to the LOGITS: the softmax uses expf,
 * is not part of the bit-exact contract and stays with the caller.  Test mode throughout: BatchNorm's mu and var are constants
 * (their slots are written as +0), gamma and beta are parameters, Dropout is the identity, the neighbour lists are constants.
 * idx1, x1, idx2, x2, pooled: the forward's intermediates, ALL FIVE or NONE; with none, fx3d_dgcnn_forward runs first, into the
 * workspace.  gx2 (256,N,B) and gx1 (64,N,B), the gradients at x2 and x1, are optional outputs (NULL: kept in the workspace).
 * Per cloud b, all of it the forward's own bits:  p = pooled[:,b];  a4 = relu(BN4(W4 p + b4)) (512);  a5 = relu(BN5(W5 a4 + b5))
 * (256);  a3[c,n] = relu(BN3(conv_3(x2)[c,n]));  sd_l = sqrtf(var_l + 1f-5).  Every operation is rounded to Float32; every chain
 * is one fmaf accumulator from +0.0f over ALL terms in the stated order, no term skipped because it is zero except in the gather.
 *   head:  d6[o] = glogits[o,b];  g5[i] = chain over o ascending, acc = fmaf(d6[o], W6[o,i], acc);  d5[i] = a5[i] > 0 ? g5[i] : +0;
 *     dz5 = (d5 gamma5) / sd5;  g4[i] = chain over o, fmaf(dz5[o], W5[o,i], acc);  d4[i] = a4[i] > 0 ? g4[i] : +0;
 *     dz4 = (d4 gamma4) / sd4;  gp[c] = chain over o, fmaf(dz4[o], W4[o,c], acc).
 *   maximum over the points:  n*(c,b) = the smallest n with a3[c,n,b] == pooled[c,b] (Float32 comparison), defined only where
 *     pooled[c,b] > 0.  A NaN or non-positive pooled value, or one that no point reproduces (a pooled that did not come from this
 *     forward), has no winner and passes nothing.  d3[c,b] = gp[c] where a winner exists, else +0;  dz3 = (d3 gamma3) / sd3.
 *     Deviation from the reference, as for the EdgeConv adjoints' maximum over k: NNlib's CPU max-pool adjoint is said to give the
 *     gradient to the first element that is approximately the maximum, cuDNN gives it to an argmax; neither can be run here to
 *     settle it.  Here it goes to the first point that EQUALS the maximum.
 *   conv_3's input gradient, a gather:  gx2[i,n,b] = the chain over the channels c with n*(c,b) == n, c ascending, of
 *     fmaf(dz3[c,b], W3[i,c], acc);  +0 for a point that wins no channel.  The terms of channels won elsewhere are not formed:
 *     in the dense product they are dz3 = +-0 times W3, which changes a chain that began at +0 only where W3 is not finite (0 * Inf
 *     is NaN) -- the gather differs from the dense product for non-finite weights only.
 *   parameter sums over the clouds, each element ONE chain over b ascending from +0:
 *     H6[o,i] = fmaf(d6[o,b], a5[i,b], acc), h6[o] = sum_b d6[o,b] (Float32 additions from +0);  H5 with d5, a4;  H4 with d4, p;
 *     H3[i,c] = fmaf(x2[i, n*(c,b), b], d3[c,b], acc) and h3[c] = sum d3[c,b], both over the clouds that have a winner for c.
 *   the families are "EdgeConv parameter adjoint"'s, verbatim:  dbeta = h;  db = (h gamma) / sd;  dW = (H gamma) / sd;
 *     dgamma = (acc + (b - mu) h) / sd with acc the chain over the input index ascending of fmaf(W, H, acc).  fc_6 has no
 *     BatchNorm: dW6 = H6, db6 = h6.
 *   the two stages:  fx3d_edgeconv_grad itself on the ec2 slice with x = x1, idx = idx2, out = x2, gout = gx2 gives the ec2 slice of
 *     gparams and gx1; again on the ec1 slice with x, idx1, x1, gout = gx1 it gives the ec1 slice and, if asked for, gx.  Their
 *     sums have the order "EdgeConv parameter adjoint" states.
 * gparams, gx, gx2 and gx1 are bit-identical to the restatement tests/dgcnn_grad_ref.py and from run to run, whatever the launch
 * shape: no float atomics, no scatter.
 * Envelope, refusals, their order, status codes and messages are fx3d_dgcnn_forward's: a NULL required pointer (params_dev, x,
 * glogits, gparams, ws), some but not all of the five intermediates, num_classes outside [1, 2^20], a bad K, N or B, a short
 * workspace or one not 256-byte aligned is FX3D_ERR_INVALID_ARG; each comes before any device work.
 * Launches on `s` only (the forward where no intermediates are given, the argmax recomputation of conv_3, the head's adjoint, the
 * two gathers, the sums over the clouds and their finishing, the two fx3d_edgeconv_grad calls), no host synchronisation, no host
 * memory read after the argument check (Capture: fx3d_dgcnn_grad: replayed).
 * ws: fx3d_dgcnn_grad_workspace_bytes(N, B, K, num_classes) -- the forward's intermediates and probabilities; per (tile of 64
 * points, channel) the first point that reproduces pooled; n*, a4, a5, d5, d4, d3, dz3; H and h of fc_4 and fc_5; gx2 and gx1; and
 * one scratch region, the largest of fx3d_dgcnn_workspace_bytes and the two stages' fx3d_edgeconv_grad_workspace_bytes, which
 * use it in turn. */
/* Batch axis: fx3d_dgcnn_grad_workspace_bytes, fx3d_dgcnn_grad: B <= 65535 -- as fx3d_dgcnn_forward. */
FX3D_API fx3d_status fx3d_dgcnn_grad_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_dgcnn_grad(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N, int32_t B,
                                     const int32_t *idx1, const float *x1, const int32_t *idx2, const float *x2,
                                     const float *pooled, const float *glogits, float *gparams, float *gx, float *gx2, float *gx1,
                                     void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- PointNet adjoint: the gradients of (m::PointNet)(X) with respect to its parameters and to X, test mode -----------------------
 * gparams = d sum(glogits . logits) / d params for logits = fx3d_pointnet_forward(x), a flat Float32 buffer with the layout of
 * params_dev (fx3d_pointnet_param_count floats), and, if gx != NULL, gx (3,N,B) = the same derivative with respect to x.  The
 * arguments up to B are the forward's.  glogits (num_classes,B) is the gradient at the LOGITS as the forward returns them, that is
 * after cls's relu: the softmax stays with the caller, as for DGCNN.  Test mode throughout: BatchNorm's mu and var are constants
 * (their slots are written as +0), gamma and beta are parameters, Dropout is the identity.  The call runs the forward's three
 * rounds itself, into its workspace (the forward does not expose the transform nets' pooled vectors).  Optional outputs (NULL: kept
 * in the workspace): gstn (3,3,B) and gfstn (64,64,B), the gradients at the two transforms; gh (64,N,B), the gradient at
 * conv_block1's output h, both paths summed; gxt (3,N,B), the gradient at x T.
 * Names are tests/pointnet_ref.py's (forward / stn_stage); sd = sqrtf(var + 1f-5); every operation is rounded to Float32; a chain
 * is one fmaf accumulator from +0.0f over all terms in the stated order, a sum one accumulator of Float32 additions from +0.
 *   relu:  passes the gradient where its OUTPUT is > 0 (Float32 compare; NaN passes nothing), else +0.
 *   BatchNorm:  passes (g gamma) / sd.
 *   conv or dense with relu, then BatchNorm (stn / fstn conv1..3 and dense2, feat.conv1, feat.dense1, feat.dense2):  forward
 *     r = relu(z + b), y = gamma ((r - mu) / sd) + beta, upstream gy.   dbeta = sum gy;   dgamma = the chain of
 *     fmaf(gy, (r - mu) / sd, acc);   d = r > 0 ? (gy gamma) / sd : +0;   db = sum d;   dW[c,o] = the chain of fmaf(a_in[c], d[o], acc)
 *     (dense layers: fmaf(d[o], a_in[i], acc)).  Nothing divides by gamma.  feat.conv2 (BatchNorm only): the same with r = z + b
 *     and no mask.  stn / fstn.dense1 (relu only): d = r > 0 ? g : +0.  dense3: d = g.  cls: d = logits > 0 ? glogits : +0.
 *     conv_block1 (BatchNorm, then relu): "EdgeConv parameter adjoint"'s formulas verbatim from H[c,o] = the chain of
 *     fmaf(x_t[c], d[o], acc) and h[o] = sum d[o], d = h > 0 ? gh : +0.
 *   the way back through a layer:  the gradient at its input i = the chain over ALL its outputs o ascending of fmaf(d[o], W[i,o], acc)
 *     (conv W[i,o] is W (Cin,Cout); dense W[o,i]).
 *   maximum over the points, in each of the three rounds:  n*(c,b) = the smallest n whose activation EQUALS the round's pooled
 *     value (Float32 ==, so -0 equals +0).  A NaN pooled value has no winner and passes nothing.  There is no "pooled > 0"
 *     condition: in stn / fstn a channel whose relu is zero at every point still has a winner, the first point; its dbeta and dgamma
 *     are then generally non-zero, its db and dW +0.  gy of conv3 is the head's gradient at the winner, and r the winner's.
 *     Deviation from the reference: the note of "DGCNN adjoint" (NNlib and cuDNN cannot be consulted here) applies verbatim.
 *   conv3's input gradient (feat: conv2's), the gather of "DGCNN adjoint":  per point the chain over the channels c it wins, c
 *     ascending, of fmaf(d[c,b], W[i,c], acc); +0 for a point that wins nothing.
 *   conv3's parameter sums run over the clouds that have a winner only, at the winner: one chain (sum) over b ascending.
 *   transforms:  x_t[j,n] = sum_i x[i,n] T[i,j,b].   gT[i,j,b] = the chain over n of fmaf(x[i,n,b], gxt[j,n,b], acc);  the path into
 *     x is the chain over j ascending of fmaf(gxt[j,n], T[i,j,b], acc).  The same for F with h and 64.  T[i,j,b] = d3[K i + j]: the
 *     gradient at dense3's output is gT re-indexed.
 *   sums of paths, one Float32 addition per element in this order:  gh = (the feat path through F) + (the fstn path);
 *     gx = (gxt through T) + (the stn path).
 * The order of every sum over points and clouds is part of the contract and depends on (N, B, num_classes) alone -- not on the
 * device, the launch shape, the workspace or the run.  A tile is FX3D_POINTNET_GRAD_TILE = 64 consecutive points of one cloud (the
 * last tile of a cloud may be shorter).
 *   the convolutions below a round's last (stn / fstn conv1 and conv2, feat.conv1, conv_block1) and gT, gF:  per tile ONE chain
 *     (sum) from +0 over the tile's points ascending; then one sum of Float32 additions from +0 over the tile values, b ascending,
 *     within b the tiles ascending (gT and gF: over the tiles of cloud b).  The families are formed after the sums (conv_block1).
 *   the dense layers and their BatchNorms, and the rounds' last convolutions:  one chain (sum) over b ascending.
 *   (So a batch is not the sum of its clouds' separate results, and N > 64 is not one chain.)
 * gparams, gx and the four optional outputs are bit-identical to the restatement tests/pointnet_grad_ref.py and from run to run:
 * no float atomics, no scatter with more than one writer.
 * Envelope, refusals, their order, status codes and messages are fx3d_pointnet_forward's: a NULL required pointer (params_dev, x,
 * glogits, gparams, ws), num_classes outside [1, 2^20], N or B below 1, B above 65535, N B above 2^31, a short workspace or one not
 * 256-byte aligned (fx3d_dgcnn_grad's alignment) is FX3D_ERR_INVALID_ARG; each comes before any device work.
 * Launches on `s` only (the forward's five launches below the classifier's head; per round the head's adjoint, the trunk's
 * adjoint, the last convolution's sums, the head's sums over the clouds, the chains over the tile partials), no host
 * synchronisation, no host memory read after the argument check (Capture: fx3d_pointnet_grad: replayed).
 * ws: fx3d_pointnet_grad_workspace_bytes(N, B, num_classes) -- h, T, F; per round and (tile, channel) the maximum, its first point
 * and the BatchNorm's input there; the head's vectors; the last convolution's input rows at the winners (128,1024,B); one partial
 * per tile and cloud; the feat path's gradient at h; gxt, gT and gF. */
#define FX3D_POINTNET_GRAD_TILE 64 /* points of one cloud whose rows are summed as one chain ("PointNet adjoint") */
/* Batch axis: fx3d_pointnet_grad_workspace_bytes, fx3d_pointnet_grad: B <= 65535 -- as fx3d_pointnet_forward. */
FX3D_API fx3d_status fx3d_pointnet_grad_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_pointnet_grad(const float *params_dev, int32_t num_classes, const float *x, int32_t N, int32_t B,
                                        const float *glogits, float *gparams, float *gx, float *gstn, float *gfstn, float *gh,
                                        float *gxt, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- PointNet training-mode forward: (m::PointNet)(X) with Flux's BatchNorm and Dropout(0.4) in training mode ----------------
 * The network, the layouts and all arithmetic but BatchNorm's statistics are "PointNet inference" above.  Every one of the 13
 * BatchNorms normalises by the mean and the uncorrected variance of what it is given over the current batch -- m = N B values per
 * channel for the nine after a 1x1 convolution, m = B for the four after a dense layer -- and the running statistics Flux
 * would then hold are returned.  What a BatchNorm is given: relu(conv + bias) in stn, fstn and feat.bn1; conv + bias in
 * conv_block1.bn and feat.bn2; relu(dense + bias) in stn.bn4, fstn.bn4 and feat.bn3; relu(dense + bias) times the dropout
 * multiplier in feat.bn4 (Dropout sits before that BatchNorm, src/models/pointnet.jl:45-57).
 * Julia's Float32 mean and sum have no order that could be reproduced; the statistics are defined here instead.
 * Sums, in Float64 (v is the Float32 value the BatchNorm is given; v v is exact in Float64, so fused or not is the same):
 *   S1 = sum (double)v, S2 = sum (double)v (double)v, every chain from +0.0 with one rounding per addition.
 *   A convolution's BatchNorm, per channel: the points of a cloud in tiles of 64 (tile k: points 64 k .. 64 k + 63; rows beyond
 *     the cloud's last point take no part).  Within a tile the rows p = 0 .. 63 whose bit 2 is h form chain h, h = 0, 1, in
 *     ascending p; the tile's sum is chain(0) + chain(1).  The tile sums t = tile + ntiles b (ntiles = ceil(N / 64)) are then
 *     folded as FX3D_POINTNET_STAT_GROUPS chains, chain g over t = g, g + 32, g + 64, ... ascending, and the chains are added
 *     in ascending g (a chain without a tile is +0.0).
 *   A dense layer's BatchNorm, per channel: one chain over the clouds in ascending b.
 *   The orders depend on (N, B) alone, never on the launch shape; no atomics.
 * Mean and variance, in Float64:  mu64 = S1 / m;  var64 = S2 / m - mu64 mu64, and 0 where that is below 0 (a NaN stays);
 *   mu = Float32(mu64), var = Float32(var64).  The normalisation is "PointNet inference"'s BatchNorm at (mu, var).
 * Running statistics, in Float32, one rounding per operation, nothing fused, with mtm = momentum:
 *   mu'  = ((1 - mtm) mu_run) + (mtm mu);   var' = ((1 - mtm) var_run) + (((mtm Float32(m)) / Float32(m - 1)) var).
 * Statistics layout (batch_stats and running, fx3d_pointnet_stat_count floats = 2 x 4928): per BatchNorm in forward order --
 *   stn.bn1 .. bn4, conv_block1.bn, fstn.bn1 .. bn4, feat.bn1 .. bn4, the order of the mu / var slots of params_dev -- mu (C), then var (C).
 * dropout: (256,B) Float32 multipliers applied with one Float32 multiplication to relu(feat.dense2); NULL: the identity.
 * batch_stats is required; running is optional and is computed from the mu / var slots of params_dev, which is not written.
 * probs (required), logits, stn, fstn, pooled (optional) as in fx3d_pointnet_forward.  logits, stn, fstn, pooled, batch_stats
 * and running are bit-identical to the restatement tests/pointnet_train_ref.py and from run to run.  fx3d_pointnet_forward on
 * parameters whose mu / var slots hold batch_stats gives, with dropout NULL, the same logits, stn, fstn and pooled bit for bit.
 * Refusals, FX3D_ERR_INVALID_ARG, before any device work: a NULL required pointer; fx3d_pointnet_forward's size limits;
 * B < 2 (a dense BatchNorm's running variance divides by B - 1); momentum not finite or outside [0, 1]; a short workspace or
 * one not 16-byte aligned.  32 launches on `s`, no host synchronisation, no host memory read after the argument check
 * (Capture: fx3d_pointnet_forward_train: replayed).  ws: fx3d_pointnet_train_workspace_bytes(N, B, num_classes) -- the forward's workspace, the tile sums
 * (2,1024,ntiles,B) Float64, and the heads' (512,B) and (256,B) activations. */
#define FX3D_POINTNET_STAT_GROUPS 32 /* chains the tile sums of a layer are folded in ("PointNet training-mode forward") */
FX3D_API fx3d_status fx3d_pointnet_stat_count(int64_t *count);
/* Batch axis: fx3d_pointnet_train_workspace_bytes, fx3d_pointnet_forward_train: B <= 65535 -- as fx3d_pointnet_forward. */
FX3D_API fx3d_status fx3d_pointnet_train_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_pointnet_forward_train(const float *params_dev, int32_t num_classes, const float *x, int32_t N,
                                                 int32_t B, const float *dropout, float momentum, float *probs, float *logits,
                                                 float *stn, float *fstn, float *pooled, float *batch_stats, float *running,
                                                 void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- PointNet training-mode adjoint: the gradients of fx3d_pointnet_forward_train with respect to its parameters and to X --------
 * gparams = d sum(glogits . logits) / d params for logits = fx3d_pointnet_forward_train(x, dropout), and, if gx != NULL, gx (3,N,B).
 * mu and var of all 13 BatchNorms are functions of the batch (their slots of gparams are written as +0: the running statistics do not
 * enter this forward), the dropout multipliers are constants.  params_dev .. B, dropout: the forward's.  batch_stats (required,
 * fx3d_pointnet_stat_count floats): what fx3d_pointnet_forward_train returned for the same (params_dev, x, dropout); the statistics
 * are not computed again.  glogits, gparams, gx, gstn, gfstn, gh, gxt: as in fx3d_pointnet_grad.  The call runs the forward's three
 * rounds itself with the test-mode kernels at batch_stats, which is what the training-mode forward's closing passes are: the
 * activations are the forward's bit for bit.
 * Everything "PointNet adjoint" states and this section does not change holds verbatim: the relu's mask on its OUTPUT, the way back
 * as one chain over ALL outputs ascending, the transforms' gT / gF and the sums of paths in their order, n*(c,b) the first point that
 * EQUALS the pooled value, no "pooled > 0" condition, every operation rounded to Float32, sd = sqrtf(var + 1f-5).
 *   BatchNorm, given v (m values per channel: N B after a convolution, B after a dense layer), xh = (v - mu) / sd, upstream gy:
 *     dbeta64 = sum (double)gy,  dgamma64 = sum (double)gy (double)xh  (the product is exact), chains from +0.0, one rounding per
 *     addition; dbeta = Float32(dbeta64), dgamma = Float32(dgamma64).  Orders:
 *       a convolution's BatchNorm below a round's last one, and conv_block1.bn:  "PointNet training-mode forward"'s order of S1 / S2
 *         verbatim (two chains per tile of 64, the tile sums in FX3D_POINTNET_STAT_GROUPS interleaved chains);
 *       a dense layer's BatchNorm:  one chain over b ascending;
 *       a round's last BatchNorm (gy is the head's gradient at the winner n*(c,b), +0 elsewhere):  one chain over b ascending over
 *         the clouds that have a winner, xh the winner's.
 *     The gradient at v:  mb = Float32(dbeta64 / m), mg = Float32(dgamma64 / m) (Float64 divisions);  t = gy - mb;  t = t - (xh mg),
 *       a multiplication and a subtraction, nothing fused;  gv = (t gamma) / sd.  At a round's last BatchNorm gy = +0 at a point that
 *       does not win the channel, so every point has a gv: the last convolution's input gradient is dense, not a gather.
 *   relu below a BatchNorm (stn / fstn conv1..3, dense2, feat.conv1, dense1, dense2):  d = r > 0 ? gv : +0 with r the relu's own output.
 *     feat.conv2 (BatchNorm only): d = gv.  conv_block1 (BatchNorm, then relu): gy = h > 0 ? gh : +0, v = conv + bias, d = gv; its
 *     families are plain sums here: dW[c,o] the chain of fmaf(x_t[c], d[o], acc), db = sum d (nothing is formed after the sums).
 *   Dropout (feat, between relu(dense2) and its BatchNorm):  the gradient below the multiplier is gv mask, one Float32 multiplication;
 *     the relu below masks on its own output.  dropout = NULL: no multiplication.
 *   The rounds' last convolutions (stn / fstn conv3, feat.conv2), sums over ALL points:  per cloud ONE chain over its points n
 *     ascending -- dW[i,o]: fmaf(a_in[i,n], d[o,n], acc); db[o]: Float32 additions -- from +0, then one sum of Float32 additions from
 *     +0 over b ascending (FX3D_POINTNET_GRAD_TRAIN_CLOUD_CHAINS: the cloud is the chain, not the 64-point tile).
 *   Every other parameter sum (the convolutions below, conv_block1, gT, gF; the dense layers: one chain over b) keeps
 *     "PointNet adjoint"'s Float32 tile orders.
 * The orders depend on (N, B, num_classes) alone; no atomics; gparams, gx and the four optional outputs are bit-identical to the
 * restatement tests/pointnet_grad_train_ref.py and from run to run.  An all-1.0f dropout gives the bits of dropout = NULL.
 * Refusals, FX3D_ERR_INVALID_ARG, each before any device work: a NULL required pointer (params_dev, x, batch_stats, glogits, gparams,
 * ws); fx3d_pointnet_forward's size limits; B < 2; a short workspace or one not 256-byte aligned.
 * Launches on `s` only, no host synchronisation, no host memory read after the argument check (Capture: fx3d_pointnet_grad_train:
 * replayed).
 * ws: fx3d_pointnet_grad_train_workspace_bytes(N, B, num_classes) -- fx3d_pointnet_grad's forward part and head vectors; the Float64
 * tile sums (2,128,ntiles,B); the last convolution's input and the gradient at it, (128,N,B) each; two (64,N,B) gradients, the feat
 * path's gradient at h; dW and db of the last convolution per cloud, (128,1024,B) and (1024,B); one partial per tile and cloud. */
#define FX3D_POINTNET_GRAD_TRAIN_CLOUD_CHAINS 1 /* chains per cloud of a last convolution's dW / db ("PointNet training-mode adjoint") */
/* Batch axis: fx3d_pointnet_grad_train_workspace_bytes, fx3d_pointnet_grad_train: B <= 65535 -- as fx3d_pointnet_forward. */
FX3D_API fx3d_status fx3d_pointnet_grad_train_workspace_bytes(int32_t N, int32_t B, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_pointnet_grad_train(const float *params_dev, int32_t num_classes, const float *x, int32_t N, int32_t B,
                                              const float *dropout, const float *batch_stats, const float *glogits, float *gparams,
                                              float *gx, float *gstn, float *gfstn, float *gh, float *gxt, void *ws, size_t ws_bytes,
                                              fx3d_stream_t s);

/* ---- DGCNN / EdgeConv training-mode forward: (m::DGCNN)(X) and (m::EdgeConv)(X) with Flux's BatchNorm and Dropout(0.5) in training mode --
 * The networks, the layouts and all arithmetic but BatchNorm's statistics are "DGCNN inference" / "EdgeConv inference" above.  Every
 * block is conv-or-dense, BatchNorm, relu, so the value v a BatchNorm is given is always the Float32 conv + bias or dense + bias,
 * before the relu.  Every BatchNorm normalises by the mean and the uncorrected variance of v over the current batch, and the running
 * statistics Flux would then hold are returned.
 * Sums, mean and variance, running update: "PointNet training-mode forward"'s, word for word.  Float64 S1 = sum (double)v,
 *   S2 = sum (double)v (double)v (exact products), every chain from +0.0 with one rounding per addition;  mu64 = S1 / m;
 *   var64 = S2 / m - mu64 mu64, and 0 where that is below 0 (a NaN stays);  mu = Float32(mu64), var = Float32(var64);  the
 *   normalisation is the inference BatchNorm at (mu, sqrtf(var + 1f-5));  in Float32, one rounding per operation, nothing fused,
 *   mu' = ((1 - mtm) mu_run) + (mtm mu),  var' = ((1 - mtm) var_run) + (((mtm Float32(m)) / Float32(m - 1)) var).
 * m per BatchNorm: K N B for an EdgeConv's BatchNorms (every edge row (k, n, b) is one value) -- DGCNN's ec1.bn1 .. bn3 (32, 64, 64
 *   channels) and ec2.bn1, bn2 (128, 256);  N B for conv3.bn (1024);  B for fc4.bn (512) and fc5.bn (256).
 * Orders of the sums.  They depend on (layers, K, N, B) alone, never on the launch shape; no atomics.  A tile is 64 consecutive
 *   points of one cloud (tile t: points 64 t .. 64 t + 63); rows beyond the cloud's last point take no part.
 *   An EdgeConv BatchNorm, per channel:  within a tile the rows p = 0 .. 63 with p div 32 = q and bit 2 of p equal to h form the
 *     chain (q, h), q, h = 0, 1: it runs over the neighbour rank k ascending and, within a k, over its 16 rows in ascending p.  The
 *     tile's sum is (chain(0,0) + chain(0,1)) + (chain(1,0) + chain(1,1)).  (A layer of up to 64 channels has the two q on
 *     different waves, a wider one in one lane: the order is the same.)  The tile sums t = tile + ntiles b are folded as
 *     "PointNet training-mode forward" folds them: FX3D_POINTNET_STAT_GROUPS chains, chain g over t = g, g + 32, ... ascending,
 *     added in ascending g.
 *   conv3.bn: "PointNet training-mode forward"'s order of a convolution's BatchNorm, verbatim (chains h = 0, 1 by bit 2 of p over
 *     the tile's 64 rows ascending, chain(0) + chain(1), the same fold).
 *   fc4.bn, fc5.bn: one chain over the clouds in ascending b.
 * Dropout: Dropout(0.5) follows relu(BN(fc_4)) and relu(BN(fc_5)) (src/models/dgcnn.jl:105-108,136-139).  dropout4 (512,B) and
 *   dropout5 (256,B) are the Float32 multipliers, applied with one Float32 multiplication each; NULL: the identity.  No random
 *   numbers are drawn on the device.  fc5.bn's statistics are therefore those of fc_5's dense layer on dropout4 . relu(BN(fc_4)).
 * Neighbours: an EdgeConv's lists are fx3d_knn_ws's on its input, as in inference, and constants (the reference's @nograd).  DGCNN's
 *   idx1 is therefore the test-mode list; idx2 is searched on the training-mode x1 and differs from test mode.
 * Statistics layout (batch_stats and running): per BatchNorm in forward order mu (C), then var (C).  EdgeConv: bn1 .. bnL,
 *   fx3d_edgeconv_stat_count = 2 (c1 + ... + cL) floats.  DGCNN: ec1.bn1 .. bn3, ec2.bn1, bn2, conv3.bn, fc4.bn, fc5.bn -- the order
 *   of the mu / var slots of params_dev -- 2336 channels, fx3d_dgcnn_stat_count = 4672 floats; its ec1 / ec2 slices are the two
 *   stages' own buffers.
 * batch_stats is required; running is optional and is computed from the mu / var slots of params_dev, which is not written.
 * fx3d_edgeconv_forward_train: params_dev .. idx_in, out, idx_out as in fx3d_edgeconv_forward, over its whole envelope (1 <= L <= 4,
 *   F <= 128, widths <= 256, no multiple of 4 or 32 required, lists searched or given).  B = 1 is allowed: K + 1 <= N gives m >= 2.
 * fx3d_dgcnn_forward_train: params_dev .. B and probs (required), logits, idx1, x1, idx2, x2, pooled (optional) as in
 *   fx3d_dgcnn_forward.  Its two stages are fx3d_edgeconv_forward_train on the ec1 / ec2 slices, bit for bit.
 * out, idx, logits, idx1, x1, idx2, x2, pooled, batch_stats and running are bit-identical to the restatement
 * tests/dgcnn_train_ref.py and from run to run.  fx3d_dgcnn_forward / fx3d_edgeconv_forward on parameters whose mu / var slots
 * hold batch_stats give, with the dropouts NULL, the same outputs bit for bit: the closing passes are those kernels.
 * Refusals, each before any device work: the forward's own limits with its status codes (FX3D_ERR_UNSUPPORTED for layers outside
 * the envelope, FX3D_ERR_INVALID_ARG for sizes);  FX3D_ERR_INVALID_ARG for a NULL required pointer (params_dev, x, probs / out,
 * batch_stats, ws), B < 2 for DGCNN (a dense BatchNorm's running variance divides by B - 1), momentum not finite or outside [0, 1],
 * a short workspace or one not 256-byte aligned.
 * Launches on `s` only, no host synchronisation, no host memory other than `layers` read and none after the argument check
 * (Capture: fx3d_edgeconv_forward_train, fx3d_dgcnn_forward_train: replayed).  Per EdgeConv: the search where idx_in is NULL, per BatchNorm a statistics pass (the forward's loop over k
 * stopped at that layer, the sums taken in the MFMA accumulators: no (K N, C, B) array in memory) and a finishing kernel, then the
 * forward's kernel at the statistics.  DGCNN: that twice, conv_3's statistics pass, finishing kernel and maxima kernel, and the head
 * in three kernels with two dense-statistics kernels between them: 20 launches besides the two searches.
 * ws: fx3d_edgeconv_train_workspace_bytes / fx3d_dgcnn_train_workspace_bytes -- the forward's workspace, the Float64 tile sums
 * (2,C,ntiles,B) of the widest layer, and for DGCNN the head's (512,B) and (256,B) dense outputs. */
FX3D_API fx3d_status fx3d_edgeconv_stat_count(const int32_t *layers, int32_t nlayers, int64_t *count);
/* Batch axis: fx3d_edgeconv_train_workspace_bytes, fx3d_edgeconv_forward_train, fx3d_dgcnn_train_workspace_bytes,
 * fx3d_dgcnn_forward_train: B <= 65535 -- as fx3d_edgeconv_forward and fx3d_dgcnn_forward. */
FX3D_API fx3d_status fx3d_edgeconv_train_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N, int32_t B,
                                                         size_t *bytes);
FX3D_API fx3d_status fx3d_edgeconv_forward_train(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K,
                                                 const float *x, int32_t N, int32_t B, const int32_t *idx_in, float momentum,
                                                 float *out, int32_t *idx_out, float *batch_stats, float *running, void *ws,
                                                 size_t ws_bytes, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_dgcnn_stat_count(int64_t *count);
FX3D_API fx3d_status fx3d_dgcnn_train_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_dgcnn_forward_train(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N,
                                              int32_t B, const float *dropout4, const float *dropout5, float momentum, float *probs,
                                              float *logits, int32_t *idx1, float *x1, int32_t *idx2, float *x2, float *pooled,
                                              float *batch_stats, float *running, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- EdgeConv training-mode adjoint: the gradients of fx3d_edgeconv_forward_train with respect to its parameters, and to X ------
 * gparams = d sum(gout . out) / d params for out = fx3d_edgeconv_forward_train(x): the function that is trained, every BatchNorm
 * at the statistics of the batch, the gradient going through mu and var.  gparams and gx as in "EdgeConv parameter adjoint" (the
 * layout of params_dev; gx (F,N,B) optional); the mu / var slots of gparams are written as +0: the running statistics do not
 * enter this forward.  The neighbours are constants.
 * batch_stats (required): fx3d_edgeconv_stat_count floats in the forward's layout, what fx3d_edgeconv_forward_train returned for the
 * same (params_dev, x, idx).  idx == NULL: the search runs as in the forward.  out == NULL: the forward's closing pass
 * (fx3d_edgeconv_forward's kernel at batch_stats) runs first, into the workspace.
 * Notation of "EdgeConv parameter adjoint"; mu_l, var_l are batch_stats', sd_l = sqrtf(var_l + 1f-5), m = K N B.  Every operation
 * is rounded to Float32 and nothing is fused unless it says fmaf.
 * Forward quantities, for every edge row (b, n, k) and layer l, the forward's bits (its closing pass is fx3d_edgeconv_forward's
 * kernel at batch_stats):
 *   v_l = z_l + b_l;   xh_l = (v_l - mu_l) / sd_l;   a_l = relu((gamma_l xh_l) + beta_l).
 * The maximum:  gy_L[k,n,o] = gout[o,n] at the smallest k with a_L[k,n,o] == out[o,n], where out[o,n] > 0, else +0 -- verbatim
 *   "EdgeConv input adjoint", including what it says about NaN and non-positive out.
 * Per layer, l = L .. 1:
 *   dbeta64_l[o] = sum (double)gy_l,  dgamma64_l[o] = sum (double)gy_l (double)xh_l (the product of two Float32 is exact), Float64
 *     sums in the order below, every chain from +0.0 with one rounding per addition.  Rows beyond a cloud's last point add nothing.
 *     At layer L a row that is not the chosen one adds nothing (a select: its xh does not enter).  At a hidden layer every valid row
 *     takes part, with gy = +0 where a_l is not positive.  gparams gets dbeta_l = Float32(dbeta64_l), dgamma_l = Float32(dgamma64_l).
 *   mb = Float32(dbeta64 / m), mg = Float32(dgamma64 / m), Float64 divisions.
 *   t = gy - mb;  t = t - (xh mg);  gv_l = (t gamma_l) / sd_l, for EVERY row of the cloud, those the relu zeroed too;  gv of a row
 *     beyond a cloud's last point is +0.
 *   dW_l[c,o] = the chain acc = fmaf(a_{l-1}[c], gv_l[o], acc);  db_l[o] = the sum of gv_l[o] -- in exactly the orders "EdgeConv
 *     parameter adjoint" gives H_l and h_l (chunks of FX3D_EDGECONV_GRAD_CHUNK, tiles, k, the permutation, the two h chains, then the
 *     chunks as one chain over (b, chunk)), and written as they come out of that sum.  (Every bias sits under a batch-statistic
 *     BatchNorm: db is the rounding noise of a sum whose exact value is 0.)
 *   for l >= 2:  d_{l-1}[c] = one fmaf chain from +0.0f over ALL o ascending of gv_l[o] W_l[c,o];  gy_{l-1} = a_{l-1} > 0 ? d_{l-1} : +0.
 * gx from d_0 (the chain of gv_1 with W_1) as "EdgeConv input adjoint" forms it: S over k ascending, then S[f] - S[F+f].
 * Order of the Float64 sums.  It depends on (layers, K, N, B) alone.  A half-tile is 32 consecutive points of one cloud (half-tile
 *   t: points 32 t .. 32 t + 31).  Per (channel, half-tile, cloud) two chains, selected by bit 2 of the point's position p in the
 *   half-tile; each runs over the neighbour rank k ascending and, within a k, over its 16 rows in ascending p; the half-tile's
 *   value is chain(0) + chain(1).  The values t = half-tile + nhalf b, nhalf = ceil(N / 32), are folded as "PointNet training-mode
 *   forward" folds tile sums: FX3D_POINTNET_STAT_GROUPS chains, chain g over t = g, g + 32, ... ascending, added in ascending g.
 * gparams and gx are bit-identical to the restatement tests/edgeconv_grad_train_ref.py and from run to run; no atomics, no
 * (K N, ., B) array in memory.
 * Envelope, refusals, their order, status codes and messages are fx3d_edgeconv_grad's, with batch_stats among the required
 * pointers (params_dev, layers, x, batch_stats, gout, gparams, ws); B = 1 is allowed, as in the forward.  Every refusal comes
 * before any device work.  Launches on `s` only (the search and / or the closing forward where idx / out are NULL, the weight
 * transpose, per layer a sums pass and a finishing kernel, the closing pass, the chain over the chunks), no host synchronisation,
 * no host memory other than `layers` read (Capture: fx3d_edgeconv_grad_train: replayed).
 * ws: fx3d_edgeconv_grad_train_workspace_bytes -- the input adjoint's, one partial of param_count floats per chunk and cloud, the
 * Float64 half-tile sums (2,C,nhalf,B) of the widest layer, and the means. */
/* Batch axis: fx3d_edgeconv_grad_train_workspace_bytes, fx3d_edgeconv_grad_train: B <= 65535 -- as fx3d_edgeconv_forward. */
FX3D_API fx3d_status fx3d_edgeconv_grad_train_workspace_bytes(const int32_t *layers, int32_t nlayers, int32_t K, int32_t N,
                                                              int32_t B, size_t *bytes);
FX3D_API fx3d_status fx3d_edgeconv_grad_train(const float *params_dev, const int32_t *layers, int32_t nlayers, int32_t K,
                                              const float *x, int32_t N, int32_t B, const int32_t *idx, const float *out,
                                              const float *batch_stats, const float *gout, float *gparams, float *gx, void *ws,
                                              size_t ws_bytes, fx3d_stream_t s);

/* ---- DGCNN training-mode adjoint: the gradients of fx3d_dgcnn_forward_train with respect to its parameters and to X --------------
 * gparams = d sum(glogits . logits) / d params for logits = fx3d_dgcnn_forward_train(x, dropout4, dropout5), and, if gx != NULL, gx
 * (3,N,B).  mu and var of all 8 BatchNorms are functions of the batch (their slots of gparams are written as +0: the running
 * statistics do not enter this forward); the dropout multipliers and both neighbour lists are constants.  params_dev .. B, dropout4,
 * dropout5 (either or both may be NULL): the forward's.  idx1, x1, idx2, x2, pooled and batch_stats (fx3d_dgcnn_stat_count floats,
 * the forward's layout) are required: what fx3d_dgcnn_forward_train returned for the same (params_dev, x, dropout4, dropout5);
 * nothing of the forward is computed again but the head's vectors.  glogits (num_classes,B); gx2 (256,N,B) and gx1 (64,N,B): the
 * gradients at x2 and x1, optional outputs.  Float32 throughout, Float64 for the BatchNorm sums; every operation is rounded and
 * nothing is fused unless it says fmaf; sd = sqrtf(var + 1f-5) at batch_stats' var.
 *   BatchNorm back, given v (m values per channel), xh = (v - mu) / sd and the upstream gy -- "PointNet training-mode adjoint"'s:
 *     dbeta64 = sum (double)gy, dgamma64 = sum (double)gy (double)xh (exact products), chains from +0.0;  dbeta = Float32(dbeta64),
 *     dgamma = Float32(dgamma64);  mb = Float32(dbeta64 / m), mg = Float32(dgamma64 / m);  t = gy - mb;  t = t - (xh mg);
 *     gv = (t gamma) / sd.
 *   1. The head.  Every block is dense, BatchNorm, relu, then the multiplier.  v4 = fc_4's dense + bias of pooled, r4 = relu(BN(v4)),
 *     in5 = r4 dropout4;  v5, r5, in6 likewise from in5: the forward's bits (its fmaf chains over the inputs ascending).  The gradient
 *     at in6 is one fmaf chain over the classes ascending of glogits[o] W6[o,i];  it is multiplied by dropout5 (one multiplication),
 *     then masked by the relu's own output: gy5 = r5 > 0 ? . : +0.  xh5 = (v5 - mu) / sd;  fc5.bn's sums are one chain over b
 *     ascending, m = B;  gv5.  The gradient at in5 is one fmaf chain over fc_5's 256 outputs ascending of gv5[o] W5[o,i];  times
 *     dropout4, masked by r4: gy4;  fc4.bn likewise with v4;  gv4.  gp[c] = one fmaf chain over fc_4's 512 outputs of gv4[o] W4[o,c].
 *     dW[o,i] = the fmaf chain over b ascending of gv[o,b] in[i,b], db[o] = the Float32 sum over b ascending of gv[o,b], for fc_4
 *     (gv4, pooled), fc_5 (gv5, in5) and fc_6 (glogits, in6), written as they come out: gv already carries gamma / sd.
 *   2. The maximum.  n*(c,b) is "DGCNN adjoint"'s: the first point n with relu(BN(conv_3(x2)))[c,n,b] == pooled[c,b] where
 *     pooled[c,b] > 0, otherwise no winner.  gy3[c,n,b] = gp[c,b] at n = n*(c,b), +0 everywhere else (the relu above conv3.bn
 *     passes at a winner: pooled > 0).  xh3 = (v3 - mu) / sd with v3 = conv_3 + bias, the forward's bits.  conv3.bn's sums are one
 *     chain over the clouds that have a winner, ascending b, of gp and gp xh3(n*);  m = N B.
 *   3. conv_3, dense.  gv3[c,n,b] = the BatchNorm back of (gy3, xh3) for EVERY point of every cloud: non-zero at the points that do
 *     not win and in the clouds without a winner; +0 beyond a cloud's last point.  No relu mask below it.
 *     gx2[i,n,b] = one fmaf chain from +0 over ALL 1024 outputs c ascending of gv3[c,n,b] W3[i,c].
 *     dW3[i,c]: per cloud ONE fmaf chain from +0 over its points n ascending of x2[i,n,b] gv3[c,n,b];  db3[c]: per cloud one chain of
 *     Float32 additions over n ascending;  then one sum of Float32 additions from +0 over b ascending
 *     (FX3D_POINTNET_GRAD_TRAIN_CLOUD_CHAINS, as PointNet's last convolutions).
 *   4. The stages.  fx3d_edgeconv_grad_train on (ec2, x1, idx2, out = x2, gout = gx2), which gives gx1, then on (ec1, x, idx1,
 *     out = x1, gout = gx1), which gives gx; each on its slice of params_dev, batch_stats and gparams, bit for bit.
 * The orders depend on (N, B, K, num_classes) alone; no atomics; gparams, gx, gx2 and gx1 are bit-identical to the restatement
 * tests/dgcnn_grad_train_ref.py and from run to run.  All-1.0f multipliers give the bits of NULL.
 * Refusals, FX3D_ERR_INVALID_ARG, each before any device work: a NULL required pointer (params_dev, x, idx1, x1, idx2, x2, pooled,
 * batch_stats, glogits, gparams, ws); fx3d_dgcnn_forward_train's size limits, B < 2 among them; a short workspace or one not
 * 256-byte aligned.  Launches on `s` only, no host synchronisation, no host memory read after the argument check
 * (Capture: fx3d_dgcnn_grad_train: replayed) -- the winners' kernel, the head in three kernels with a cloud-sums kernel after each, three dense-sums kernels,
 * conv_3's two dense kernels and two chains over the clouds, then the two stages' launches.
 * ws: fx3d_dgcnn_grad_train_workspace_bytes(N, B, K, num_classes) -- the per-tile first matches (1024,ntiles,B) with what conv3.bn
 * was given there; the head's vectors; dW3 and db3 per cloud, (256,1024,B) and (1024,B); gx2 and gx1; one scratch region, the
 * larger of the two stages' fx3d_edgeconv_grad_train workspaces. */
/* Batch axis: fx3d_dgcnn_grad_train_workspace_bytes, fx3d_dgcnn_grad_train: B <= 65535 -- as fx3d_dgcnn_forward. */
FX3D_API fx3d_status fx3d_dgcnn_grad_train_workspace_bytes(int32_t N, int32_t B, int32_t K, int32_t num_classes, size_t *bytes);
FX3D_API fx3d_status fx3d_dgcnn_grad_train(const float *params_dev, int32_t num_classes, int32_t K, const float *x, int32_t N,
                                           int32_t B, const float *dropout4, const float *dropout5, const int32_t *idx1,
                                           const float *x1, const int32_t *idx2, const float *x2, const float *pooled,
                                           const float *batch_stats, const float *glogits, float *gparams, float *gx, float *gx2,
                                           float *gx1, void *ws, size_t ws_bytes, fx3d_stream_t s);

/* ---- Training step: what the loop of examples/pointnet_classification.jl / dgcnn_classification.jl does around the model ------------
 *   loss(x, y) = crossentropy(m(x), y);  opt = Flux.ADAM(lr);  gs = gradient(ps) do ... end;  Flux.update!(opt, ps, gs)
 * Three entry points between and after fx3d_*_forward_train and fx3d_*_grad_train.  Nothing is fused (-ffp-contract=off), every
 * operation below is rounded once, in the precision named.  Float32 and int32 arrays may be aligned to 4 bytes only; the Float64
 * and UInt64 arrays (loss, betap, counter_dev) must be 8-byte aligned, FX3D_ERR_INVALID_ARG otherwise.  Launches on `s` only: no
 * host synchronisation, no allocation, no host memory or environment read (Capture: fx3d_crossentropy, fx3d_dropout_mask,
 * fx3d_adam_step: replayed).  Plain stores, no atomics; the results
 * are the same bits from run to run and those of the restatement tests/train_step_ref.py (the loss up to the device's log).
 *
 * fx3d_crossentropy: Flux.crossentropy(probs, onehot(labels)) with its gradient at the logits, and the tutorial's accuracy count.
 *   probs (num_classes,B): a classifier's output.  labels: B int32 on the device, 0-based.
 *   glogits[o,b] = (probs[o,b] - [o == labels[b]]) / Float32(B): one Float32 subtraction (of 1.0f or of +0.0f), one Float32 division.
 *   loss (one Float64) = (-(sum_b log((double)probs[labels[b],b]))) / (double)B, the sum one chain from +0.0 in ascending b; log is
 *     the device's double log (not pinned to a bit pattern, as the softmax's exp is not).  probs = 0 at a label gives +Inf.
 *   counts[0]: the clouds whose first maximum over the classes is the label -- the scan best = 0; for o = 1 .. : probs[o,b] >
 *     probs[best,b] moves best to o (Julia's argmax on a column without NaN: the lowest index on a tie).
 *   counts[1]: the labels outside [0, num_classes).  Such a label adds NaN to the loss, subtracts +0.0f everywhere in its column,
 *     is never used as an index into probs and does not count in counts[0].
 *   One launch of one block.  Refusals (FX3D_ERR_INVALID_ARG): a NULL pointer, num_classes < 1, B < 1, loss not 8-byte aligned.
 *
 * fx3d_dropout_mask: the multipliers of Dropout(p) in training mode, drawn on the device: Flux's rand > p ? T(1 / q) : T(0).
 *   Element e takes word e mod 4 of philox4x32_10 on the counter (e div 4, stream_id, 0, 0) under the key (low, high half of
 *   seed + (counter_dev ? *counter_dev : 0)), the convention of fx3d_sample_points_draw;  u = (float)(word >> 8) 2^-24;
 *   out[e] = ((double)u > p) ? (float)(1.0 / (1.0 - p)) : 0.0f.  The draws are the library's, not Julia's.  fx3d_counter_add
 *   advances counter_dev between steps; stream_id tells the masks of one step apart.
 *   Refusals: out NULL, n < 0 or n > 2^34, p outside [0, 1) or NaN, stream_id < 0, counter_dev not 8-byte aligned.  n = 0: nothing is done.
 *
 * fx3d_adam_step: Flux.Optimise.ADAM(eta, (beta1, beta2)) over one flat buffer of n elements, what Flux's broadcast computes with
 *   Float64 hyper-parameters and Float32 arrays.  g: the gradient.  m, v: the optimiser's state, zero before the first step.
 *   betap: two Float64 on the device, (beta1, beta2) before the first step.  x: the parameters.  Flux's eps is 1e-8.  Per element:
 *     m <- Float32((beta1 (double)m) + ((1 - beta1) (double)g))             1 - beta1 in Float64; product, product, sum
 *     v <- Float32((beta2 (double)v) + ((1 - beta2) (double)(g (*) g)))     g (*) g the FLOAT32 product (Julia's g^2 on a Float32 array)
 *     d <- Float32((((double)m / (1 - betap[0])) / (sqrt((double)v / (1 - betap[1])) + eps)) eta)     the new m and v, as stored
 *     x <- x - d                                                            Float32
 *   with the Float64 divisions and the square root correctly rounded.  After all elements: betap <- betap .* (beta1, beta2), a
 *   running Float64 product, not a power.  So g = +0 on zero state gives d = +0 and leaves every bit of x (-0.0 too); g = 1e30f
 *   makes g (*) g, hence v, +Inf and d = 0; NaN propagates.
 *   running, stat_map, nstat (optional; nstat = 0: ignored): x[stat_map[i]] = running[i] for i < nstat -- the running statistics
 *   fx3d_*_forward_train returned, written into the mu / var slots of the parameters.  The gradient at those slots is +0 (the
 *   training-mode adjoints write it so), so ADAM's own result there is the old value; the write of `running` comes after it:
 *   The entry is two launches: the elements (betap is only read), then a finishing launch, ordered behind the first by the stream,
 *   which writes the mapped slots and advances betap.  No block reads betap while another thread writes it, and a mapped slot ends
 *   as running[i] whatever ADAM computed there.  An index of stat_map outside [0, n) is skipped.
 *   The element launch moves 28 bytes per element, as float4 where the four arrays reach a 16-byte boundary after the same number
 *   of elements (those and the tail go one by one), one by one otherwise.
 *   Refusals: n < 0, nstat < 0, a NULL g, m, v, betap or x, nstat > 0 without running and stat_map, betap not 8-byte aligned.
 *   n = 0: betap advances and nothing else happens. */
/* Batch axis: fx3d_crossentropy: unbounded -- one block walks the batch. */
FX3D_API fx3d_status fx3d_crossentropy(const float *probs, const int32_t *labels, int32_t num_classes, int32_t B, float *glogits,
                                       double *loss, int32_t *counts, fx3d_stream_t s);
FX3D_API fx3d_status fx3d_dropout_mask(int64_t n, double p, uint64_t seed, const uint64_t *counter_dev, int32_t stream_id, float *out,
                                       fx3d_stream_t s);
FX3D_API fx3d_status fx3d_adam_step(int64_t n, double eta, double beta1, double beta2, double eps, const float *g, float *m, float *v,
                                    double *betap, float *x, const float *running, const int32_t *stat_map, int64_t nstat,
                                    fx3d_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* FLUX3D_HIP_H */
