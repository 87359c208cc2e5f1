/*
 * slgpu.h -- C ABI of libslgpu.so, the MI355X (gfx950) implementation of the
 * structured-light reconstruction hot path of
 * Nuttoty/Structured_Light_for_3D_Model_Replication:
 *
 *   gray_decode(folder, n_cols, n_rows)          server/sl_system.py:508-580
 *   reconstruct_point_cloud(col, row, mask, tex, calib)  server/sl_system.py:584-653
 *   generate_cloud(scan_dir, calib_file)         server/sl_system.py:483-694
 *
 * The reference has no FFI; its boundary is the Python function triple above
 * (called from server/gui.py:563, multi_point_cloud_process.py:206-212 and
 * Old/process_cloud.py:231-233).  This header is what a ctypes binding of that
 * triple calls; see INTEGRATION.md for the binding.
 *
 * Conventions
 *  - Every entry point returns SL_OK (0) or a negative SL_E* code; the message
 *    of the last failure on a context is sl_ctx_last_error().
 *  - Pointers named "device" are HIP device pointers owned by the caller.  The
 *    library owns only the calibration tables and scratch inside a context.
 *  - A context belongs to one device; calls on one context must be serialised
 *    by the caller (one context per thread or per device).  There is no global
 *    state, so independent contexts may be used concurrently.
 *  - Work is enqueued on `stream` (a hipStream_t; NULL = default stream) and is
 *    asynchronous unless the function says otherwise.
 */
#ifndef SLGPU_H
#define SLGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL_ABI_VERSION 1

#define SL_OK 0
#define SL_EINVAL (-1)    /* bad argument -> Python ValueError                          */
#define SL_EINDEX (-2)    /* dangling odd image reached: the IndexError of
                             sl_system.py:553-554                                      */
#define SL_EHIP (-3)      /* HIP runtime failure -> RuntimeError                        */
#define SL_ENOCALIB (-4)  /* sl_set_calib not called / shape mismatch -> ValueError       */
#define SL_ETIMEOUT (-5)  /* reserved                                                     */
#define SL_ECAPACITY (-6) /* output capacity smaller than the pixel count -> ValueError   */
#define SL_EIO (-7)       /* file could not be written -> OSError                        */

/* mask_mode */
#define SL_MASK_ADAPTIVE 0 /* white > 1.5*pct95(black) & contrast > 0.05*max(contrast):
                              sl_system.py:526-535                                      */
#define SL_MASK_FIXED 1    /* white > 40 & contrast > 10:
                              multi_point_cloud_process.py:36-38, Old/process_cloud.py:47-49 */

/* xyz_dtype */
#define SL_XYZ_F32 0 /* 12 B/point, the round-to-nearest fp32 of the reference's f64   */
#define SL_XYZ_F64 1 /* 24 B/point, bit-identical to the reference's f64              */
/* 12 B/point, f32 arithmetic: per-coordinate relative error vs the reference's f64
 * <= (11 + 10*16) * 2^-24 ~ 1.0e-5 (north-star tolerance 1e-4).  Points with
 * condition number sum|n_i r_i| / |n.r| > 16 are computed exactly.  Applies when
 * Oc = 0, no Nc table and no pose; otherwise identical to SL_XYZ_F32.          */
#define SL_XYZ_F32_FAST 2

typedef struct sl_ctx sl_ctx;

int sl_abi_version(void);

/* Create a context on HIP device `device`.  Replaces nothing in the reference
 * (which keeps no state); the context holds the calibration tables. */
int sl_ctx_create(int device, sl_ctx** out);
void sl_ctx_destroy(sl_ctx* ctx);
const char* sl_ctx_last_error(const sl_ctx* ctx);

/* Pre-size the context's scratch for up to `max_views` views of `max_px`
 * pixels each (and the histograms of a whole launch group) so that later calls
 * allocate nothing (required before stream capture into a hipGraph).  Calls
 * grow scratch on demand otherwise.
 * Graphs: any sequence of calls captured on one stream replays any number of
 * times, in any order with other work on the context.  Nothing a launch group
 * accumulates into depends on the host's view of the sequence: the super-block
 * sums live in two buffers whose alternation is kept on the device (the
 * producer, k_decode or k_count, reads a selector word, accumulates into that
 * buffer and zeroes the OTHER one, whose last reader -- the previous group's
 * k_cloud -- is done; the consumer only flips the selector, so the buffer it
 * read keeps its sums until the next producer zeroes it); the adaptive mask's
 * histograms are zeroed by their last reader (an arrival counter).  The one
 * thing that crosses a call boundary, a histogram pass queued by
 * sl_stack_next, is taken only by a call in the same capture (a graph's first
 * call therefore runs its own histogram pass; a pass the graph's last call
 * queues is cleared by the next call that does not take it). */
int sl_ctx_reserve(sl_ctx* ctx, int64_t max_views, int64_t max_px);

/* Upload calibration for an H x W camera (the calib.mat fields loaded at
 * sl_system.py:493-504).  Host pointers:
 *   cam_K   3x3 row-major f64            (calib["cam_K"])
 *   Oc      3 f64                         (calib["Oc"], zeros from calibrate_final)
 *   planes  Wp x 4 row-major f64 (n0,n1,n2,d) (calib["wPlaneCol"] transposed as at
 *           sl_system.py:591)
 *   Nc      3 x (H*W) row-major f64, or NULL (calib["Nc"]).  When Nc equals the
 *           pinhole rays of cam_K bit for bit (always, for calibrate_final output)
 *           it is not uploaded and rays are recomputed on the fly; otherwise it
 *           is kept on the device and read per pixel, as sl_system.py:605-606. */
int sl_set_calib(sl_ctx* ctx, int H, int W, const double* cam_K, const double* Oc,
                 const double* planes, int Wp, const double* Nc);

/* Fused gray_decode + reconstruct_point_cloud over `n_views` views.
 *
 * stack      device, view v at stack + v*stack_view_stride: n_img planes of H*W
 *            uint8 in the reference's sorted-file order [white, black, (pattern,
 *            inverse) x bits...] (sl_system.py:510-520, 553-557).
 * n_cols/n_rows  projector stripes; ceil(log2()) gives the bit counts exactly as
 *            sl_system.py:538-539 (each must be in [1, 65536]).
 * tex_bgr    device, [H][W][3] BGR per view (the colour imread of file 0,
 *            sl_system.py:580), or NULL to use the white plane replicated.
 * poses      device, n_views x 4x4 row-major f64 applied to every point of the
 *            view (turntable merge epilogue), or NULL.
 * col_out, row_out  device int32 [n_views][H][W], full frame, unmasked (may be
 *            NULL).  mask_out device uint8 (0/1) [n_views][H][W] (may be NULL).
 * xyz_out    device, out_capacity x 3 of f32 or f64 (xyz_dtype), NULL for
 *            decode only.  bgr_out device uint8 out_capacity x 3 (NULL allowed
 *            only together with xyz_out).  Both 16-byte aligned.
 * view_offsets  device int64 [n_views+1]: points of view v occupy
 *            [view_offsets[v], view_offsets[v+1]) of the merged cloud, in
 *            ascending pixel order inside each view (np.where order,
 *            sl_system.py:601).  Required when xyz_out is given.
 * out_capacity  must be >= n_views*H*W.
 *
 * Row planes are read only if row_out is non-NULL (the cloud does not use the
 * row code: sl_system.py:584-653 reads only col_map).
 * Returns SL_EINDEX / SL_EINVAL for the stack lengths on which the reference
 * raises IndexError / ValueError. */
int sl_decode_triangulate(sl_ctx* ctx, const uint8_t* stack, int64_t stack_view_stride,
                          int n_views, int n_img, int H, int W, int n_cols, int n_rows,
                          const uint8_t* tex_bgr, int64_t tex_view_stride, int mask_mode,
                          const double* poses, int32_t* col_out, int32_t* row_out,
                          uint8_t* mask_out, void* xyz_out, int xyz_dtype, uint8_t* bgr_out,
                          int64_t out_capacity, int64_t* view_offsets, void* stream);

/* Masked-pixel counts (the "Processing {N} valid pixels..." line of
 * reconstruct_point_cloud, sl_system.py:601-602: N = np.count_nonzero(mask)):
 * arms the NEXT sl_decode_triangulate on this context (that call only; it is
 * consumed even when the call fails) to write the number of pixels of view v
 * that pass the mask into device_counts[v] (device int64 [n_views], 8-byte
 * aligned), asynchronously on that call's stream.  NULL disarms.  Without it
 * the kernels count nothing. */
int sl_mask_counts_to(sl_ctx* ctx, int64_t* device_counts);

/* Stack readiness for the NEXT sl_decode_triangulate on this context (that
 * call only; consumed even when the call fails): the stack and texture are in
 * place once `event` (a hipEvent_t recorded by the caller) has completed --
 * the call's work waits for it on its stream -- or already now when `event`
 * is NULL.  Results are unchanged.  (Round 3 ran the histogram pass of such a
 * call on a side stream beside the previous call's triangulation: measured
 * slower than sl_stack_next's pre-stats, DESIGN.md 5.2, and removed.) */
int sl_stack_ready(sl_ctx* ctx, void* event);

/* The call AFTER the coming one (a stream of views): arms the NEXT
 * sl_decode_triangulate on this context (that call only; consumed even when it
 * fails) to compute, beside its own triangulation (extra workgroups of its last
 * k_cloud launch), the adaptive-mask histograms (sl_system.py:526-528) of the
 * first launch group of `stack` [n_views][...] (view stride stack_view_stride,
 * 16-byte aligned, the same frame size as the coming call).  The call after it
 * then starts with its decode -- when it is on this context, reads that same
 * stack pointer, stride, view count and frame size with the adaptive mask,
 * nothing ran on the context in between, and both calls are enqueued in the
 * same stream capture (or both outside one); otherwise it computes its
 * histograms itself.  The caller promises that `stack` holds the next call's images, in
 * place by the time the coming call's work starts on its stream, and unchanged
 * until the next call.  Results are unchanged.  NULL disarms, and also drops a
 * pass an earlier call queued for the next one (that call then computes its
 * own histograms: e.g. after a failed graph capture of chained calls).  A
 * queued pass is taken or dropped by the very next call on the context, even
 * one that fails its argument checks (never by a later one).
 * Within one call of several launch groups (more than 65536 chunks of 1024
 * pixels) the same happens without any declaration: group g's k_cloud computes
 * group g + 1's histograms, so only the first group can need a k_stats launch. */
int sl_stack_next(sl_ctx* ctx, const uint8_t* stack, int64_t stack_view_stride, int n_views);

/* A prepared call: sl_decode_triangulate's arguments (without the stream),
 * checked once and kept, so that a stream of views through the same resident
 * buffers (a ring of stack slots, reused outputs) re-enqueues it with two
 * arguments -- what a host-bound caller of small frames spends its time on is
 * the per-call argument marshalling, not the kernels.  sl_call_run is exactly
 * sl_decode_triangulate with the kept arguments on `stream` (the same checks,
 * results and errors); the buffers must stay valid until sl_call_destroy. */
typedef struct sl_call sl_call;
int sl_call_prepare(sl_ctx* ctx, const uint8_t* stack, int64_t stack_view_stride, int n_views, int n_img,
                    int H, int W, int n_cols, int n_rows, const uint8_t* tex_bgr, int64_t tex_view_stride,
                    int mask_mode, const double* poses, int32_t* col_out, int32_t* row_out, uint8_t* mask_out,
                    void* xyz_out, int xyz_dtype, uint8_t* bgr_out, int64_t out_capacity, int64_t* view_offsets,
                    sl_call** out);
int sl_call_run(sl_call* call, void* stream);
void sl_call_destroy(sl_call* call);

/* reconstruct_point_cloud on caller-supplied maps (sl_system.py:584-653).
 * col_map device int32 [n_views][H][W]; mask device uint8 [n_views][H][W]
 * (non-zero = valid); tex_bgr device [n_views][H][W][3].  Outputs as above. */
int sl_triangulate_maps(sl_ctx* ctx, const int32_t* col_map, const uint8_t* mask,
                        const uint8_t* tex_bgr, int n_views, int H, int W,
                        const double* poses, void* xyz_out, int xyz_dtype, uint8_t* bgr_out,
                        int64_t out_capacity, int64_t* view_offsets, void* stream);

/* Synchronise `stream` and report any HIP failure of the work enqueued so far
 * on this context.  Blocking. */
int sl_sync(sl_ctx* ctx, void* stream);

/* Adaptive-mask diagnostics of the last sl_decode_triangulate (blocking):
 * noise_floor = np.percentile(black, 95) and dynamic_range = max(white-black)
 * as float32 (sl_system.py:527-528), and the integer thresholds the kernel
 * compared against (white > thr_white, contrast > thr_contrast). */
int sl_last_thresholds(sl_ctx* ctx, int view, float* noise_floor, float* dynamic_range,
                       int* thr_white, int* thr_contrast);

/* Timing: with max_calls > 0, each later call (up to that many) records HIP
 * events on its stream before k_decode, k_count, k_cloud and after the call.
 * 0 disables.  Events between kernels add launch gaps: keep them out of
 * throughput measurements. */
int sl_profile_enable(sl_ctx* ctx, int max_calls);

/* Blocking: summed event time (ms) of k_decode, k_count and k_cloud over the
 * recorded calls since the last read, and their count; restarts recording. */
int sl_profile_read(sl_ctx* ctx, double* decode_ms, double* count_ms, double* cloud_ms, int* calls);

/* The last call's kernel path -- 0: k_decode + k_count + k_cloud; 1: [k_stats]
 * + k_decode + k_cloud, k_decode applying the mask and the point decision
 * (frames with W % 16 == 0, W, H <= 4096 and Wp <= 2048; sl_profile_* and
 * sl_time_kernels then report k_stats in the k_count slot) -- its number of
 * launch groups, and the pixels of its last launch group (what
 * sl_time_kernels re-runs).  Host only. */
int sl_last_launch_info(sl_ctx* ctx, int* path, int64_t* launches, int64_t* last_launch_px);

/* Blocking, measurement only: re-launches the kernels of the last launch group
 * of the previous sl_decode_triangulate / sl_triangulate_maps call `reps`
 * times each, back to back on its stream, and returns each kernel's average
 * duration from HIP events around the `reps` launches (the events' own cost
 * amortised).  The inputs the call consumed (histograms, block sums) are
 * rebuilt once first, untimed; k_cloud and k_count run first: the call's
 * outputs are rewritten with the same values.  Afterwards the context's
 * scratch is clean again: a histogram pass queued by sl_stack_next is dropped
 * (the next call computes its own).  Eager only: SL_EINVAL while that stream
 * is capturing into a graph. */
int sl_time_kernels(sl_ctx* ctx, int reps, double* decode_ms, double* count_ms, double* cloud_ms);

/* ASCII PLY of a cloud exactly as the reference writes it (sl_system.py:665-691,
 * multi_point_cloud_process.py:121-131): header, then per point
 * "%.4f %.4f %.4f %d %d %d\n" of x, y, z and the colour swapped from BGR to
 * RGB; %.4f correctly rounded, ties to even (what Python's f"{x:.4f}" prints).
 * Host memory, host code (no device needed); formatted on `threads` threads.
 * xyz is n x 3 f32 or f64 (xyz_dtype), bgr n x 3 uint8.
 * sl_format_ply: with out == NULL only *out_len is set (the byte size). */
int sl_format_ply(const void* xyz, int xyz_dtype, const uint8_t* bgr, int64_t n, int threads, char* out,
                  int64_t out_capacity, int64_t* out_len);
/* Write that text to `path` (replaces save_ply, sl_system.py:665-691).  A
 * large regular file already at `path` is renamed away and unlinked beside the
 * write rather than truncated in place (the same file results, faster);
 * symlinks and hard-linked files are written through / truncated as
 * open(path, "w") does.  The same for sl_write_ply_device / _binary. */
int sl_write_ply(const char* path, const void* xyz, int xyz_dtype, const uint8_t* bgr, int64_t n, int threads);

/* The same file from a cloud in device memory (xyz / bgr device pointers,
 * e.g. a call's outputs): the text is formatted on the device (one thread
 * per point, the host formatter's digit code) into context scratch, copied
 * back through a pinned buffer in chunks and written, the host formatting
 * nothing; byte-identical to sl_write_ply.  A cloud with a non-finite
 * coordinate or |x| >= 9e11 (printed through libc's %.4f) is copied back and
 * formatted on the host instead.  Blocking on `stream` (hipStream_t). */
int sl_write_ply_device(sl_ctx* ctx, const char* path, const void* xyz, int xyz_dtype, const uint8_t* bgr, int64_t n,
                        void* stream);

/* Binary little-endian PLY with the same header properties (float x y z,
 * uchar red green blue; colour swapped from BGR): 15-byte records, xyz rounded
 * to float32 when xyz_dtype is SL_XYZ_F64.  A compact binary form of the
 * reference's ASCII file (the merged cloud's Open3D-layout file, double xyz
 * and normals, is ply.save_ply_open3d). */
int sl_write_ply_binary(const char* path, const void* xyz, int xyz_dtype, const uint8_t* bgr, int64_t n,
                        int threads);

/* ---- PLY reader: the body of a vertex-only PLY parsed on the device ----
 * (csrc/slplyread.inl; the header is the caller's: ply.read_cloud_device) */

/* *status of sl_parse_ply_ascii: accepted, or which condition sends the whole
 * file to the host reader */
#define SL_PLY_ACCEPTED 0
#define SL_PLY_BAD_BYTE 1           /* a byte outside 0-9 + - . e E ' ' \t \r \n ("nan", "inf", '#') */
#define SL_PLY_BAD_TOKEN 2          /* a token outside the grammar ("1e", "1.2.3")                   */
#define SL_PLY_TOKEN_COUNT 3        /* not n_rows x n_cols tokens                                     */
#define SL_PLY_RAGGED_LINE 4        /* a non-blank line without exactly n_cols tokens                 */
#define SL_PLY_COLOUR_RANGE 5       /* a colour that is no integer in 0..255 (set by the caller, who
                                       knows which columns are colours)                               */
#define SL_PLY_UNDECIDED_OVERFLOW 6 /* more undecided tokens than undecided_cap                       */

/* col_type of sl_unpack_ply_binary */
#define SL_PLY_F32 0
#define SL_PLY_F64 1
#define SL_PLY_U8 2
#define SL_PLY_I8 3
#define SL_PLY_I16 4
#define SL_PLY_U16 5
#define SL_PLY_I32 6
#define SL_PLY_U32 7

/* The ASCII body (n_bytes at body_dev, device memory, 16-byte aligned) of
 * n_rows vertices with n_cols properties into table_dev, f64 [n_rows][n_cols],
 * every token converted as strtod / Python's float() converts it (correctly
 * rounded), bit for bit.
 * Tokens are separated by ' ' \t \r \n (as rply reads them).  Grammar:
 * [+-]? digits [. digits]? ([eE] [+-]? digits)? with a digit in the mantissa
 * ("5." and ".5" are inside).  A token is +-M * 10^p, M its decimal
 * significand without leading zeros, p the net power of ten.
 * Exact tier, on the device: M <= 2^53 and |p| <= 22.  double(M) and 10^|p|
 * are exact, so double(M) / 10^|p|, double(M) * 10^p or double(M) is one
 * correctly rounded IEEE operation on exact operands (Clinger); the sign is
 * applied last ("-0.0000" is -0.0).
 * Three outcomes for a token: exact tier; UNDECIDED (inside the grammar,
 * outside the tier: appended to undecided_dev as int64 (token number, byte
 * offset, length), at most undecided_cap entries, then converted on the host
 * by strtod and patched into the table; *n_undecided is their number); or
 * outside the grammar.  The latter, and the other SL_PLY_* conditions, reject
 * the WHOLE file: *status > 0, the table's content is undefined, and the
 * caller reads the file with the host reader (whose result and exceptions are
 * then the file's).  *status == SL_PLY_ACCEPTED: the table is complete.
 * Returns SL_OK for either; SL_E* for bad arguments or a HIP failure.  Scratch
 * (8 B per token) is the context's.  Blocking on `stream` (hipStream_t). */
int sl_parse_ply_ascii(sl_ctx* ctx, const uint8_t* body_dev, int64_t n_bytes, int64_t n_rows, int n_cols,
                       double* table_dev, int64_t* undecided_dev, int64_t undecided_cap, int64_t* n_undecided,
                       int* status, void* stream);

/* The binary_little_endian body: n_rows records of `stride` bytes at body_dev
 * (device memory, no alignment asked: fields are read bytewise); property j is
 * col_type[j] (SL_PLY_*) at byte col_offset[j] of the record (host arrays of
 * n_cols) and is widened to f64 into table_dev, f64 [n_rows][n_cols].  Every
 * property must lie inside the record (SL_EINVAL).  Blocking on `stream`. */
int sl_unpack_ply_binary(sl_ctx* ctx, const uint8_t* body_dev, int64_t n_rows, int64_t stride, int n_cols,
                         const int* col_offset, const int* col_type, double* table_dev, void* stream);

/* ---- merge stage (server/processing.py:116-182) ----
 * Open3D's PointCloud::VoxelDownSample and RemoveStatisticalOutliers on a
 * device cloud (xyz f64 [n][3], bgr u8 [n][3] or NULL).  Blocking on `stream`;
 * counts are returned on the host.  Parity vs Open3D is unpinned (not in this
 * image): oracle/merge_oracle.py restates the algorithms. */

/* One point per occupied voxel of edge voxel_size, grid origin min - voxel_size/2:
 * the mean of its points (summed in ascending index, f64) and of its colours
 * (as c/255, written back as round(clamp(mean)*255)).  Output in ascending
 * voxel key (ix, iy, iz) (Open3D: hash order); out arrays hold n points.
 * SL_EINVAL for voxel_size <= 0, "voxel_size is too small." (Open3D's check),
 * or a grid over 2e6 voxels per axis. */
int sl_voxel_downsample(sl_ctx* ctx, const double* xyz, const uint8_t* bgr, int64_t n, double voxel_size,
                        double* out_xyz, uint8_t* out_bgr, int64_t* out_n, void* stream);

/* Mean distance to the nb_neighbors (<= 32) nearest points, the point itself
 * included (exact kNN, f64) -> avg_dist[n] (device); keeps
 * 0 < avg < mean + std_ratio * std (Bessel): their indices, ascending, ->
 * out_index (device, capacity n), the count -> *out_n. */
int sl_statistical_outliers(sl_ctx* ctx, const double* xyz, int64_t n, int nb_neighbors, double std_ratio,
                            double* avg_dist, int64_t* out_index, int64_t* out_n, void* stream);

/* select_by_index: out[j] = in[index[j]] (device; bgr optional).  Asynchronous. */
int sl_select_by_index(sl_ctx* ctx, const double* xyz, const uint8_t* bgr, const int64_t* index, int64_t m,
                       double* out_xyz, uint8_t* out_bgr, void* stream);

/* In place p' = M p for a row-major 4x4 pose (device), rows in the order
 * ((m0 x + m1 y) + m2 z) + m3 -- PointCloud::Transform.  Asynchronous. */
int sl_transform_points(sl_ctx* ctx, double* xyz, int64_t n, const double* pose, void* stream);

/* PointCloud::EstimateNormals(KDTreeSearchParamHybrid(radius, max_nn)) on a
 * cloud without normals (processing.py:178: radius = 2 voxel, max_nn = 30):
 * per point, the neighbours with ((dx^2 + dy^2) + dz^2) < radius^2 (itself
 * included) in ascending (distance, index), the first max_nn; covariance from
 * their cumulants (identity below 3 neighbours); normal = Open3D's
 * FastEigen3x3 eigenvector of the smallest eigenvalue, (0, 0, 1) when zero ->
 * normals [n][3] f64 (device).  max_nn <= 32.  Blocking on `stream`. */
int sl_estimate_normals(sl_ctx* ctx, const double* xyz, int64_t n, double radius, int max_nn, double* normals,
                        void* stream);

/* registration_icp(source, target, max_distance, init,
 * TransformationEstimationPointToPlane()) of merge_pro_360 (processing.py:
 * 154-156), Open3D's RegistrationICP loop: every (moved) source point's
 * nearest target point with ((dx^2 + dy^2) + dz^2) < max_distance^2 (least
 * (d^2, index)); the point-to-plane step from those correspondences (JTJ and
 * JTr folded in source order, 64-point blocks left to right; the 6x6 system
 * by a pivoted LDLT as Eigen's (Open3D's A.ldlt().solve(b): zero pivots give
 * zero components, so a rank-deficient system still moves along the
 * directions it constrains); update = [Rz Ry Rx | t] of the solution);
 * transformation = update *
 * transformation; until |d fitness| < relative_fitness and |d rmse| <
 * relative_rmse, or max_iteration steps (Open3D's defaults: 30, 1e-6, 1e-6).
 * source / target / target_normals: device f64 [n][3]; init and the returned
 * transformation: host row-major 4x4; fitness = correspondences / n_src,
 * inlier_rmse = sqrt(sum d^2 / correspondences) of the last evaluation;
 * *iterations = steps taken.  Blocking on `stream`.  Parity vs Open3D is
 * unpinned (oracle/merge_oracle.py restates this arithmetic). */
int sl_icp_point_to_plane(sl_ctx* ctx, const double* source, int64_t n_src, const double* target,
                          const double* target_normals, int64_t n_tgt, double max_distance, const double* init,
                          int max_iteration, double relative_fitness, double relative_rmse, double* transformation,
                          double* fitness, double* inlier_rmse, int* iterations, void* stream);

/* ---- loop-closing 360 merge (Old/new360Merge.py:77-137) ----
 * get_information_matrix_from_point_clouds(source, target, max_distance,
 * transformation): Open3D's GetInformationMatrixFromPointClouds restated
 * (csrc/slinfo.inl; parity with Open3D unpinned; tests/posegraph_oracle.py is
 * the CPU restatement, bit for bit).  source [n_src][3] / target [n_tgt][3]:
 * device f64.  Every source point is moved by transformation (host, row-major
 * 4x4, sl_transform_points' order; exactly the identity: not moved); its
 * correspondence is the nearest target point with d^2 < max_distance^2, lowest
 * index on ties; a correspondence with the target point (x, y, z) adds G^T G,
 * G's rows (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1), entry
 * (a, c) as (r1[a] r1[c] + r2[a] r2[c]) + r3[a] r3[c].  Sums: source points in
 * blocks of 64 consecutive indices, a left fold inside each block (unmatched
 * points skipped), the blocks' partial sums folded left to right on the host.
 * -> information host[36] (row-major, symmetric) and *correspondences (may be
 * NULL).  An empty source or target, or no correspondence: the zero matrix.
 * SL_EINVAL: NULL arguments, 2^31 points or more, max_distance <= 0,
 * non-finite target coordinates.  Blocking on `stream`. */
int sl_information_matrix(sl_ctx* ctx, const double* source, int64_t n_src, const double* target, int64_t n_tgt,
                          double max_distance, const double* transformation, double* information,
                          int64_t* correspondences, void* stream);

/* global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(),
 * criteria, GlobalOptimizationOption(reference_node)) with every edge certain
 * (csrc/slposegraph.inl states the algorithm; tests/posegraph_oracle.py
 * restates it; parity with Open3D unpinned).  Host only: no context, no GPU
 * call.  poses: n_nodes row-major 4x4 (in/out).  Edge k: edge_source[k],
 * edge_target[k], edge_transformation + 16 k (source frame -> target frame),
 * edge_information + 36 k; edge_uncertain (may be NULL): a non-zero entry is
 * SL_EINVAL, since the line process and edge pruning are not implemented.
 * Stops at the first of max|b| < min_right_term, |delta| <
 * min_relative_increment (|x| + min_relative_increment), |r - r_new| <
 * min_relative_residual_increment r, r < min_residual, max_iteration
 * (Open3D's defaults: 1e-6 each, 100; max_iteration_lm 20 retries per
 * iteration).  -> *iterations, *initial_residual, *final_residual (sum of e^T
 * Lambda e; each may be NULL).  SL_EINVAL: n_nodes < 1, reference_node or an
 * edge id out of range, NULL arguments.  The dense 6N x 6N system: 3 arrays
 * of 288 N^2 bytes. */
int sl_pose_graph_optimize(double* poses, int n_nodes, const int32_t* edge_source, const int32_t* edge_target,
                           const double* edge_transformation, const double* edge_information,
                           const uint8_t* edge_uncertain, int n_edges, int reference_node, int max_iteration,
                           int max_iteration_lm, double min_right_term, double min_relative_increment,
                           double min_relative_residual_increment, double min_residual, int* iterations,
                           double* initial_residual, double* final_residual);

/* ---- global registration (merge_pro_360's FPFH + RANSAC, processing.py:79-113) ----
 * Open3D's algorithms restated (parity unpinned: no Open3D in this image;
 * oracle/registration_oracle.py is the CPU restatement, bit-identical).
 *
 * KDTreeFlann::SearchHybrid(p, radius, max_nn) of every point of xyz [n][3]
 * (device f64): the points with ((dx^2 + dy^2) + dz^2) < radius^2 (itself
 * included) in ascending (d2, index), the first max_nn -> out_idx /
 * out_d2 [n][max_nn] and out_cnt [n] (device).  max_nn <= 1024.  Blocking.
 * Ties (a documented deviation): equal distances are ordered by index here
 * and in sl_estimate_normals / sl_compute_fpfh; nanoflann leaves them in its
 * KD-tree traversal order (an unstable sort), so with duplicate points Open3D
 * may pick another neighbour set or "self" entry.  No reference fixture covers
 * it; the oracle (oracle/registration_oracle.py) states the same rule, and
 * parity with Open3D stays unpinned. */
int sl_radius_search(sl_ctx* ctx, const double* xyz, int64_t n, double radius, int max_nn, int32_t* out_idx,
                     double* out_d2, int32_t* out_cnt, void* stream);

/* compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn))
 * (processing.py:91-94: radius 5 voxel, max_nn 100): per point its SPFH (the
 * pair features -- fdlibm acos / atan2 -- of its neighbours, 11 bins each,
 * 100 / (neighbours - 1) per pair) and the FPFH = the 1/d2-weighted sum of the
 * neighbours' SPFH, each third scaled to 100, + its own SPFH (zero for a
 * point without neighbours) -> feature [n][33] f64 (device; Open3D's
 * Feature.data_ transposed).  normals: [n][3] (estimate_normals).  Blocking. */
int sl_compute_fpfh(sl_ctx* ctx, const double* xyz, const double* normals, int64_t n, double radius, int max_nn,
                    double* feature, void* stream);

/* The nearest row of b [nb][dim] for every row of a [na][dim] (device f64;
 * dim == 33): nanoflann's L2 order (four dimensions at a time, then the
 * rest), ties to the lower index (a documented deviation: nanoflann's 1-NN
 * keeps the first candidate its tree traversal meets) -> out [na] (device
 * int32); -1 for a row with no distance below +inf (NaN features never match,
 * as nanoflann's strict compare).  Blocking. */
int sl_feature_nn(sl_ctx* ctx, const double* a, int64_t na, const double* b, int64_t nb, int dim, int32_t* out,
                  void* stream);

/* registration_ransac_based_on_feature_matching(source, target, source_feature,
 * target_feature, mutual_filter, max_distance,
 * TransformationEstimationPointToPoint(False), 3,
 * [CorrespondenceCheckerBasedOnEdgeLength(edge_similarity),
 *  CorrespondenceCheckerBasedOnDistance(max_distance)],
 * RANSACConvergenceCriteria(max_iteration, confidence)) (processing.py:98-111):
 * correspondences = feature nearest neighbours (mutual: both ways agree; fewer
 * than 0.1f * n_src mutual pairs: the one-way set; a source row without a
 * neighbour makes no pair); then Open3D's RANSAC loop
 * as one thread runs it -- iteration i draws correspondences
 * splitmix64(seed + (3 i + k + 1) * 0x9E3779B97F4A7C15) (k = 0..2; Open3D's
 * std::mt19937 draw is unseeded, so no run of it is reproducible), checks edge
 * lengths, fits Umeyama (Eigen's 3x3 JacobiSVD), checks distances, and
 * validates (fitness = source points with a target within max_distance / n,
 * inlier RMSE); the best by (fitness, then lower RMSE) updates the estimated
 * iteration count log(1 - confidence) / log(1 - inlier_ratio^3) -- evaluated
 * on the GPU in batches of hypotheses, walked in iteration order.
 * source / target [n][3], features [n][33]: device f64.  Host outputs: the
 * row-major 4x4 transformation (identity if nothing validated), fitness,
 * inlier_rmse, iterations run, validations (hypotheses that passed both
 * checkers) and the correspondence count (any output pointer but
 * transformation may be NULL).  Blocking on `stream`. */
int sl_ransac_feature_matching(sl_ctx* ctx, const double* source, int64_t n_src, const double* target, int64_t n_tgt,
                               const double* source_feature, const double* target_feature, int mutual_filter,
                               double max_distance, double edge_similarity, int max_iteration, double confidence,
                               uint64_t seed, double* transformation, double* fitness, double* inlier_rmse,
                               int* iterations, int* validations, int64_t* n_corres, void* stream);

/* ---- per-view clean-up (ProcessingLogic.remove_background, processing.py:25-52) ----
 * pcd.segment_plane(distance_threshold, ransac_n, num_iterations, probability):
 * Open3D's PointCloud::SegmentPlane as one thread runs it, restated (parity
 * vs Open3D is unpinned: not in this image; tests/plane_oracle.py is the CPU
 * restatement, bit-identical; csrc/slplane.inl states the arithmetic and the
 * one summation order).  Iteration i draws points splitmix64(seed +
 * (ransac_n i + k + 1) * 0x9E3779B97F4A7C15) (k < ransac_n; duplicates are not
 * redrawn -- Open3D samples without replacement), fits a plane (3 points: the
 * normalised cross product, a zero one skipped; 4..16: GetPlaneFromPoints),
 * counts the points with |((a x + b y) + c z) + d| < distance_threshold; the
 * best by (count, then lower rmse = err / sqrt(count)) sets the break
 * iteration k = min(log(1 - probability) / log(1 - fitness^ransac_n),
 * num_iterations) (0 for fitness 1); iteration i runs iff i <= k.  Hypotheses
 * are scored on the GPU `batch` at a time (0: 64, the fastest measured at 4K;
 * any batch gives the same bits) and walked in iteration order.
 * xyz: device f64 [n][3].  Outputs: plane_model host[4] = GetPlaneFromPoints
 * of the best hypothesis's inliers (f64 sums in the fixed order of
 * slplane.inl); their indices, ascending -> inlier_index (device, capacity
 * n), the count -> *n_inliers; the other points' indices, ascending ->
 * rest_index (device, capacity n; may be NULL; n - *n_inliers of them);
 * *iterations = iterations run (may be NULL).  No hypothesis with an inlier
 * (collinear clouds, num_iterations 0): plane (0, 0, 0, 0) and no inliers
 * (Open3D: the same zero plane, from its initial best).  SL_EINVAL for
 * ransac_n < 3 or > 16, n < ransac_n, n >= 2^31, num_iterations < 0,
 * probability outside (0, 1).  Blocking on `stream`. */
int sl_segment_plane(sl_ctx* ctx, const double* xyz, int64_t n, double distance_threshold, int ransac_n,
                     int num_iterations, double probability, uint64_t seed, int batch, double* plane_model,
                     int64_t* inlier_index, int64_t* n_inliers, int64_t* rest_index, int* iterations, void* stream);

/* The indices of [0, n) that index[0..m) (device) does not list, ascending ->
 * out_index (device, capacity n), their count -> *out_n: what
 * select_by_index(index, invert=true) gathers.  Entries outside [0, n) are
 * ignored; duplicates are allowed.  Blocking on `stream`. */
int sl_index_complement(sl_ctx* ctx, const int64_t* index, int64_t m, int64_t n, int64_t* out_index, int64_t* out_n,
                        void* stream);

/* ---- Poisson meshing (ProcessingLogic.reconstruct_stl / mesh_360, processing.py:185-311) ----
 * create_from_point_cloud_poisson as Kazhdan's FFT Poisson reconstruction on
 * a dense periodic grid of R = 2^depth nodes per axis (depth 1..10), node (i,
 * j, k) at origin + h (i, j, k), linear index (i R + j) R + k.  Open3D's is the
 * adaptive-octree variant: parity with Open3D is unpinned; csrc/slmesh.inl
 * states every stage and tests/mesh_oracle.py restates it on the CPU, bit for
 * bit except the FFT solve, which the Python side runs through torch.fft
 * (mesh.py).  All pointers are device memory unless noted; every call blocks
 * on `stream`.
 *   sl_mesh_splat          trilinear splat of n (< 2^31) points: 64-bit
 *                          fixed-point (2^-30) integer atomic adds into acc
 *                          [4][R^3] (weight, then w n_x, w n_y, w n_z), which
 *                          the caller has zeroed.  origin: host[3].
 *   sl_mesh_unfix          out[i] = float(double(acc[i]) 2^-30), i < count.
 *   sl_mesh_divergence     periodic central differences of V [3][R^3] (f32).
 *   sl_mesh_sample         trilinear value (f64) of an f32 grid at n points.
 *   sl_ordered_sum         slplane.inl's ordered sum of v[stride i + offset],
 *                          i < n -> *sum (host).
 *   sl_orient_normals      orient_normals_towards_camera_location, in place:
 *                          a normal with n . (location - p) < 0 is negated, a
 *                          zero normal becomes the unit vector towards
 *                          location ((0, 0, 1) at the location itself).
 *                          location: host[3].
 *   sl_mesh_extract_count  marching tetrahedra, pass 1: emask [R^3] (the
 *                          crossed edges a node owns), vpos / tpos [R^3] (the
 *                          first vertex of a node, the first triangle of a
 *                          cube) and the totals (host); SL_ECAPACITY at 2^31.
 *   sl_mesh_extract_emit   pass 2, into vertices f64 [n_vertices][3] and
 *                          triangles int32 [n_triangles][3].
 *   sl_mesh_remove_vertices  remove_vertices_by_mask: mask u8 [n_vertices]
 *                          (non-zero: remove); outputs have the inputs'
 *                          capacity, the new counts -> host. */
int sl_mesh_splat(sl_ctx* ctx, const double* xyz, const double* normals, int64_t n, int depth, const double* origin,
                  double h, int64_t* acc, void* stream);
int sl_mesh_unfix(sl_ctx* ctx, const int64_t* acc, int64_t count, float* out, void* stream);
int sl_mesh_divergence(sl_ctx* ctx, const float* V, int depth, double h, float* div, void* stream);
int sl_mesh_sample(sl_ctx* ctx, const float* grid, int depth, const double* origin, double h, const double* xyz,
                   int64_t n, double* out, void* stream);
int sl_ordered_sum(sl_ctx* ctx, const double* v, int64_t n, int64_t stride, int64_t offset, double* sum,
                   void* stream);
int sl_orient_normals(sl_ctx* ctx, const double* xyz, double* normals, int64_t n, const double* location,
                      void* stream);
int sl_mesh_extract_count(sl_ctx* ctx, const float* chi, int depth, double iso, uint8_t* emask, uint32_t* vpos,
                          uint32_t* tpos, int64_t* n_vertices, int64_t* n_triangles, void* stream);
int sl_mesh_extract_emit(sl_ctx* ctx, const float* chi, int depth, double iso, const double* origin, double h,
                         const uint8_t* emask, const uint32_t* vpos, const uint32_t* tpos, int64_t n_vertices,
                         int64_t n_triangles, double* vertices, int32_t* triangles, void* stream);
int sl_mesh_remove_vertices(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, const uint8_t* mask, double* out_vertices, int32_t* out_triangles,
                            int64_t* out_n_vertices, int64_t* out_n_triangles, void* stream);

/* ---- mesh clean-up (csrc/slmeshclean.inl, which states the definitions) ----
 * Open3D's cluster_connected_triangles / remove_triangles_by_mask /
 * remove_unreferenced_vertices / simplify_vertex_clustering(Average), restated
 * in order-free forms; tests/meshclean_oracle.py is their CPU form and the
 * results equal it exactly.  vertices f64 [n_vertices][3], triangles int32
 * [n_triangles][3] (device); n_vertices < 2^31, 3 n_triangles < 2^32.  A pass of
 * its own reads every index first: one outside 0 .. n_vertices - 1 is SL_EINDEX
 * and nothing is indexed.  Outputs are sized by the caller to the input's size;
 * the true counts -> host.  Zero triangles / vertices succeed.  Blocking on
 * `stream`.
 *   sl_mesh_cluster_triangles    two triangles are adjacent iff they share an
 *       edge (the unordered pair); a cluster is a connected component; its label
 *       is the rank of its smallest triangle index among the clusters' smallest
 *       indices.  -> triangle_clusters int32 [n_triangles], cluster_n_triangles
 *       int64 [capacity n_triangles], the count -> *n_clusters; cluster_area f64
 *       [capacity n_triangles] may be NULL (then `vertices` may be NULL too and
 *       the sort by label is not run): the triangle areas in ascending index in
 *       blocks of 64 from the cluster's first member, left folds from 0.0.
 *       Lock-free union-find on the device; nothing spins.
 *   sl_mesh_cluster_triangles_stats    the calling thread's last call's host
 *       milliseconds per stage (edge keys, sort, union, flatten + rank, counts,
 *       areas; stage_ms[capacity], zero-filled) -- a measurement aid.
 *   sl_mesh_remove_triangles     mask u8 [n_triangles] (non-zero: remove); the
 *       rest keep their order.  No index is read as an index.
 *   sl_mesh_remove_unreferenced  the vertices of no triangle go, the rest keep
 *       their order; out_triangles [n_triangles] re-indexed.
 *   sl_mesh_simplify_clustering  sl_voxel_downsample's grid over all vertices
 *       (its limits and messages; a non-finite vertex is SL_EINVAL); a voxel's
 *       new index is the rank of its smallest member vertex, its vertex the mean
 *       of its members summed in ascending index; triangles mapped, dropped when
 *       two indices are equal, rotated so that the smallest index comes first,
 *       the first occurrence of every triple kept, in input order. */
int sl_mesh_cluster_triangles(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                              int64_t n_triangles, int32_t* triangle_clusters, int64_t* cluster_n_triangles,
                              double* cluster_area, int64_t* n_clusters, void* stream);
int sl_mesh_cluster_triangles_stats(double* stage_ms, int capacity);
int sl_mesh_remove_triangles(sl_ctx* ctx, const int32_t* triangles, int64_t n_triangles, const uint8_t* mask,
                             int32_t* out_triangles, int64_t* out_n_triangles, void* stream);
int sl_mesh_remove_unreferenced(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                                int64_t n_triangles, double* out_vertices, int32_t* out_triangles,
                                int64_t* out_n_vertices, void* stream);
int sl_mesh_simplify_clustering(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                                int64_t n_triangles, double voxel_size, double* out_vertices, int32_t* out_triangles,
                                int64_t* out_n_vertices, int64_t* out_n_triangles, void* stream);

/* ---- mesh output (csrc/slmeshwrite.inl, which states the arithmetic) ----
 * o3d.io.write_triangle_mesh for .stl and .ply after compute_vertex_normals(),
 * from a mesh in device memory: vertices f64 [n_vertices][3], triangles int32
 * [n_triangles][3], both counts < 2^31.  Every index is checked on the device
 * first: one outside 0 .. n_vertices - 1 is SL_EINDEX, and a writer then
 * neither creates nor touches `path`.  Blocking on `stream`.
 *   sl_mesh_triangle_normals   out f64 [n_triangles][3]: (p1 - p0) x (p2 - p0)
 *       over its length, zero for a zero length: the bits of
 *       tests/mesh_oracle.py's triangle_normals.
 *   sl_mesh_vertex_normals     out f64 [n_vertices][3]: per vertex the sum over
 *       its triangles of llrint(unit normal 2^40) in wrapping 64-bit integers,
 *       normalised; (0, 0, 1) for a zero sum.  Deviation: Open3D sums in f64 in
 *       triangle order.  Exact against tests/meshwrite_oracle.py.
 *   sl_write_stl_device        binary STL: 80 zero bytes, the count, 50-byte
 *       records (float32 normal and corners, a zero attribute).
 *   sl_write_mesh_ply_device   binary little-endian PLY in Open3D's layout:
 *       double x y z nx ny nz per vertex, uchar 3 + three uint per face.
 *     The records are packed on the device and come back through a ring of two
 *     pinned chunks of `chunk_triangles` triangles (0: 655 360, i.e. 32 768 000
 *     bytes; other values are rounded up to a multiple of 256; at most 8 times
 *     the default), kept with the context: staging does not grow with the mesh.
 *     The file is opened as sl_write_ply opens it.  SL_EIO: the file could not
 *     be opened or written; SL_EHIP: a launch or copy failed (nothing more is
 *     queued after it).  path NULL packs and copies without a file (measurement).
 *   sl_mesh_write_stats        the calling thread's last writer call: host
 *       milliseconds waiting for chunks, in write(), and in all (stage_ms
 *       [capacity], zero-filled) -- a measurement aid. */
int sl_mesh_triangle_normals(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                             int64_t n_triangles, double* out, void* stream);
int sl_mesh_vertex_normals(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                           int64_t n_triangles, double* out, void* stream);
int sl_write_stl_device(sl_ctx* ctx, const char* path, const double* vertices, int64_t n_vertices,
                        const int32_t* triangles, int64_t n_triangles, int64_t chunk_triangles, void* stream);
int sl_write_mesh_ply_device(sl_ctx* ctx, const char* path, const double* vertices, int64_t n_vertices,
                             const int32_t* triangles, int64_t n_triangles, int64_t chunk_triangles, void* stream);
int sl_mesh_write_stats(double* stage_ms, int capacity);

/* ---- vertex colours (csrc/slmeshcolor.inl, which states the definition; the
 * coloured PLY is written by csrc/slmeshwrite.inl, with the other writers) ----
 * Open3D's Poisson returns vertex_colors when the cloud has colours and its PLY
 * writer stores them as uchar red green blue; restated order-free (parity with
 * Open3D is unpinned; exact against tests/meshcolor_oracle.py).  Blocking on
 * `stream`; scratch from the merge stage's pool.
 *   sl_mesh_transfer_colors   cloud_xyz f64 [n][3], cloud_bgr u8 [n][3],
 *       query_xyz f64 [m][3] (device); n, m < 2^31.  Tier t has radius radius 2^t;
 *       a query's tier is the first whose open ball holds a cloud point, and its
 *       colour the blend of the up to k (1..16) points of least (d2, index) in
 *       that ball with weights d2_first / d2_i, or the first point's colour when
 *       d2_first == 0.  Tiers run until the radius exceeds the diagonal of the
 *       joint bounding box, or max_tiers of them (< 0: no cap).  A non-finite
 *       query, an empty cloud and a query without a point by the last tier get
 *       fill_bgr (host [3]) and tier 255.  -> out_bgr u8 [m][3], out_tier u8 [m]
 *       (may be NULL).  A non-finite cloud coordinate, a radius that is not
 *       finite and positive, k outside 1..16: SL_EINVAL.  m == 0 and n == 0
 *       succeed.
 *   sl_mesh_transfer_colors_stats   the calling thread's last call (stats
 *       [capacity], zero-filled; a measurement aid): [0] tiers run, [1] queries
 *       filled, [2] host milliseconds in the grid builds, [3] in the query
 *       passes, [4 + t] queries resolved in tier t, t < 16, [20] tiers that ran
 *       one wave per query (the upper tiers' kernel; the results are the same).
 *   sl_write_mesh_ply_colors_device   sl_write_mesh_ply_device with bgr u8
 *       [n_vertices][3] (device): the header gains property uchar red, green,
 *       blue after nz and the vertex record has 51 bytes, the six doubles and
 *       then red green blue from the BGR storage.  Same index check (the path is
 *       untouched on SL_EINDEX), same ring (its slots hold `chunk_triangles`
 *       vertices of 51 bytes). */
int sl_mesh_transfer_colors(sl_ctx* ctx, const double* cloud_xyz, const uint8_t* cloud_bgr, int64_t n,
                            const double* query_xyz, int64_t m, double radius, int k, int max_tiers,
                            const uint8_t* fill_bgr, uint8_t* out_bgr, uint8_t* out_tier, void* stream);
int sl_mesh_transfer_colors_stats(double* stats, int capacity);
int sl_write_mesh_ply_colors_device(sl_ctx* ctx, const char* path, const double* vertices, int64_t n_vertices,
                                    const int32_t* triangles, int64_t n_triangles, const uint8_t* bgr,
                                    int64_t chunk_triangles, void* stream);

/* ---- mesh smoothing (csrc/slmeshsmooth.inl, which states the definitions) ----
 * Open3D's compute_adjacency_list / filter_smooth_simple / filter_smooth_laplacian
 * / filter_smooth_taubin for the vertices, restated order-free (parity with
 * Open3D is unpinned; exact against tests/meshsmooth_oracle.py).  vertices f64
 * [n_vertices][3], triangles int32 [n_triangles][3] (device); n_vertices < 2^31,
 * 6 n_triangles < 2^32.  A pass of its own reads every index first: one outside
 * 0 .. n_vertices - 1 is SL_EINDEX and nothing is indexed.  Zero triangles /
 * vertices succeed.  Blocking on `stream`; scratch from the merge stage's pool.
 *   sl_mesh_adjacency   N(v): the indices that share a triangle with v ((a, a, b)
 *       puts a into its own set), as CSR: row_start int64 [n_vertices + 1],
 *       neighbours int32 [capacity 6 n_triangles], every row ascending without
 *       duplicates, the entry count -> *n_neighbours.  boundary u8 [n_vertices]
 *       (may be NULL): 1 for a vertex with an edge {v, w}, w != v, that is the
 *       side of exactly one (triangle, side) pair.
 *   sl_mesh_smooth      method 0 simple: p' = (p + the neighbours in ascending
 *       index) / (1 + |N|); 1 laplacian: `iterations` steps p' = p + lambda (sum_j
 *       w_j p_j / sum_j w_j - p), w_j = 1 / (|p - p_j| + 1e-12), folded in
 *       ascending neighbour index; 2 taubin: a lambda step then a mu step per
 *       iteration.  Every step reads the previous step's positions; iterations
 *       0 copies.  A vertex with an empty row keeps its position; with
 *       fixed_boundary != 0 so does every boundary vertex.  -> out_vertices f64
 *       [n_vertices][3], which must not overlap `vertices`.  A non-finite vertex,
 *       negative iterations, a non-finite lambda (methods 1, 2) or mu (method 2),
 *       another method: SL_EINVAL.
 *   sl_mesh_smooth_stats   the calling thread's last call of either: host
 *       milliseconds per stage (keys, sort, CSR, iterations; stage_ms[capacity],
 *       zero-filled) -- a measurement aid. */
int sl_mesh_adjacency(sl_ctx* ctx, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                      int64_t* row_start, int32_t* neighbours, uint8_t* boundary, int64_t* n_neighbours,
                      void* stream);
int sl_mesh_smooth(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                   int64_t n_triangles, int method, int iterations, double lambda, double mu, int fixed_boundary,
                   double* out_vertices, void* stream);
int sl_mesh_smooth_stats(double* stage_ms, int capacity);

/* ---- mesh checks (csrc/slmeshcheck.inl, which states the definitions) ----
 * Open3D's is_edge_manifold / is_vertex_manifold / is_orientable / is_watertight,
 * get_non_manifold_edges / _vertices, orient_triangles, get_surface_area,
 * get_volume, remove_degenerate_triangles and remove_duplicated_triangles,
 * restated order-free (parity with Open3D is unpinned; exact against
 * tests/meshcheck_oracle.py).  triangles int32 [n_triangles][3], vertices f64
 * [n_vertices][3] (device); n_vertices < 2^31, 3 n_triangles < 2^32.  A pass of
 * its own reads every index first: one outside 0 .. n_vertices - 1 is SL_EINDEX
 * and nothing is indexed.  Zero triangles succeed.  Blocking on `stream`;
 * scratch from the merge stage's pool.
 *   Sides: (a, b, c) has a->b, b->c, c->a; a side's key is min n_vertices + max,
 *   its direction bit from < to.  A triangle with two equal indices is
 *   degenerate and still gives its three sides to the edge counts.  An edge of
 *   m sides: m = 1 boundary, m = 2 regular (consistent iff the direction bits
 *   differ), m >= 3 non-manifold.  Corners (t, k) at one vertex are joined iff
 *   their (non-degenerate) triangles share an edge that contains the vertex; a
 *   vertex whose corners fall into more than one class is non-manifold.
 *   Orientable: no m >= 3 edge and a flip bit per triangle that makes every
 *   m = 2 edge consistent (two loops {v, v} never are).
 *   sl_mesh_check   one sort of the sides, everything from it.  counts (host,
 *       int64 [8]): 0 unique edges, 1 boundary edges, 2 non-manifold edges,
 *       3 inconsistent edges, 4 non-manifold vertices, 5 degenerate triangles,
 *       6 orientable (0 / 1), 7 rows of the edge list.  Optional device outputs
 *       (NULL: skipped, and so is their gather): edges int32 [rows][2], (min,
 *       max) in ascending key order -- the m >= 3 edges, and with
 *       allow_boundary_edges == 0 the m = 1 edges too (room for n_triangles rows,
 *       or 3 n_triangles without boundary edges allowed); vertices int32
 *       [counts[4]], ascending (room for n_vertices); oriented int32
 *       [n_triangles][3]: per component (connected through m = 2 edges) the
 *       smallest triangle index keeps its winding, a flipped (a, b, c) is
 *       (a, c, b); a copy when the mesh is not orientable.
 *   sl_mesh_check_stats   the calling thread's last sl_mesh_check or
 *       sl_mesh_measure: host milliseconds per stage (side keys, sort, classify
 *       and edge list, corner classes, parity unions, flips, measures;
 *       stage_ms[capacity], zero-filled) -- a measurement aid.
 *   sl_mesh_measure   A_t = 0.5 sqrt((n0 n0 + n1 n1) + n2 n2), n = (v1 - v0) x
 *       (v2 - v0); W_t = ((x0 c0 + y0 c1) + z0 c2) / 6.0, c = v1 x v2 (f64,
 *       uncontracted); *area and *signed_volume (host) are their ordered sums
 *       (sl_ordered_sum) in triangle order.  The signed volume means a volume only
 *       on a watertight mesh (the caller checks) and is positive iff the
 *       windings face outward.  A non-finite vertex: SL_EINVAL.
 *   sl_mesh_remove_degenerate   the triangles with two equal indices go, the
 *       rest keep their order -> out_triangles (room for n_triangles rows).
 *   sl_mesh_remove_duplicated_triangles   every triple is rotated so that its
 *       strictly smallest index comes first (the opposite winding is another
 *       triple); the first occurrence of every rotated triple is kept, in input
 *       order and as it was given -> out_triangles (room for n_triangles rows). */
int sl_mesh_check(sl_ctx* ctx, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                  int allow_boundary_edges, int64_t* counts, int32_t* edges, int32_t* vertices, int32_t* oriented,
                  void* stream);
int sl_mesh_check_stats(double* stage_ms, int capacity);
int sl_mesh_measure(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                    int64_t n_triangles, double* area, double* signed_volume, void* stream);
int sl_mesh_remove_degenerate(sl_ctx* ctx, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                              int32_t* out_triangles, int64_t* out_n_triangles, void* stream);
int sl_mesh_remove_duplicated_triangles(sl_ctx* ctx, const int32_t* triangles, int64_t n_triangles,
                                        int64_t n_vertices, int32_t* out_triangles, int64_t* out_n_triangles,
                                        void* stream);

/* ---- mesh hole filling (csrc/slmeshfill.inl, which states the definitions) ----
 * The boundary components of a mesh and caps for the ones that are plain loops;
 * definitions of this library's own (Open3D's tensor fill_holes is unpinned),
 * exact against tests/meshfill_oracle.py and independent of any traversal or
 * atomic order.  Inputs, limits and the index pass as for the mesh checks; a
 * non-finite vertex is SL_EINVAL.  Blocking on `stream`; scratch from the
 * merge stage's pool.
 *   A boundary side is a side a->b whose edge has that one side (m = 1).  Sides
 *   that share an end vertex are one component; its label is its smallest
 *   vertex, its size its number of sides, its extent the diagonal of the box of
 *   its vertices.  A vertex is simple iff one boundary side leaves and one
 *   enters it; a component all of whose vertices are simple is a simple loop.
 *   A simple loop is filled iff 3 <= size <= 2^22, size <= max_hole_edges and
 *   extent <= hole_size (a negative limit: none; hole_size is inclusive): a
 *   loop a->b->c->a of three sides, a the label, gets the triangle (a, c, b); a
 *   longer one gets one new vertex at its centroid (64-bit fixed-point sums)
 *   and the triangle (b, a, centre) per side a->b.
 *   counts (host, int64 [8]), of both calls: 0 components, 1 simple loops,
 *   2 filled loops, 3 skipped components that are not simple, 4 simple loops not
 *   filled (over a limit, or fewer than three sides), 5 new vertices, 6 new
 *   triangles, 7 boundary sides of the input.  sl_mesh_boundary_loops counts
 *   what a fill without limits would do.
 *   sl_mesh_boundary_loops   one row per component in ascending label ->
 *       out_label int32, out_size int64, out_simple uint8, out_extent f64 (NULL
 *       when vertices is NULL), device, room for counts[0] rows; with all four
 *       NULL only the counts are computed, which is how a caller sizes them.
 *   sl_mesh_fill_holes   out_vertices f64 [n_vertices + counts[5]][3]: the old
 *       vertices, then the centroids in ascending label; out_triangles int32
 *       [n_triangles + counts[6]][3]: the old triangles, then the new ones in
 *       ascending from-vertex a (the triangle of a three-sided loop at its
 *       label).  Room for n_vertices + components and n_triangles + boundary
 *       sides rows always suffices; with both NULL only the counts are computed.
 *   sl_mesh_fill_stats   the calling thread's last call of either: host
 *       milliseconds per stage (side keys, sort, boundary sides, unions, per-loop
 *       sums, caps or rows; stage_ms[capacity], zero-filled) -- a measurement aid. */
int sl_mesh_boundary_loops(sl_ctx* ctx, const int32_t* triangles, int64_t n_triangles, const double* vertices,
                           int64_t n_vertices, int32_t* out_label, int64_t* out_size, uint8_t* out_simple,
                           double* out_extent, int64_t* counts, void* stream);
int sl_mesh_fill_holes(sl_ctx* ctx, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                       int64_t n_triangles, int64_t max_hole_edges, double hole_size, double* out_vertices,
                       int32_t* out_triangles, int64_t* counts, void* stream);
int sl_mesh_fill_stats(double* stage_ms, int capacity);

/* ---- consistent tangent-plane normal orientation (processing.py:201, :282) ----
 * orient_normals_consistent_tangent_plane restated on the kNN graph alone
 * (csrc/slorient.inl; tests/orient_oracle.py is the CPU restatement, bit for
 * bit).  Open3D adds Delaunay-EMST edges, which connect the graph; this does
 * not, so every connected component is oriented on its own, and parity with
 * Open3D is unpinned.  normals [n][3] (device f64) are oriented IN PLACE; each
 * comes out exactly +n or -n.
 *   graph   idx [n][k], cnt [n] as sl_radius_search writes them.  Slot s = i k +
 *           j names the entry (i, idx[i][j]); every slot with j < cnt[i] and
 *           idx[i][j] != i is an undirected edge candidate.  n k < 2^32.
 *   weight  dot = (nx mx + ny my) + nz mz (f64, uncontracted); w = 1 - |dot|
 *           where that is > 0, else 0.
 *   order   (w, slot): strict and total, so the minimum spanning forest is
 *           unique as a set of slots.
 *   parity  an edge flips iff dot < 0.
 *   root    per component the point of largest z (lowest index on ties); the
 *           component is negated iff the root's nz < 0; every other point's
 *           sign is the XOR of the flipping edges on its tree path to the root.
 * tree_slots (device, [n], or NULL) receives the forest's slots, one per point
 * that is not the last of its component to be merged, in ascending order of
 * that point (the same in every run; sort it to compare sets); their number ->
 * *n_tree and the number of components -> *n_components (host; n_tree +
 * n_components = n).  n == 0 succeeds and writes nothing.  SL_EINVAL: k < 1,
 * NULL arguments, n >= 2^31, n k >= 2^32.  Boruvka rounds with parity-carrying
 * union-find; the host reads a counter per round and a flag per pointer jump,
 * both bounded by ceil(log2 n) + 2 (SL_EHIP "internal error" beyond, never a
 * spin).  Scratch: 8 n k bytes (a key per slot) + 30 n.  Blocking on `stream`.
 * sl_orient_normals_mst_stats: the calling thread's last call's rounds and the
 * jump launches of each (jumps[capacity], zero-filled) -- a measurement aid. */
int sl_orient_normals_mst(sl_ctx* ctx, const double* xyz, double* normals, int64_t n, const int32_t* idx,
                          const int32_t* cnt, int k, uint32_t* tree_slots, int64_t* n_tree, int64_t* n_components,
                          void* stream);
int sl_orient_normals_mst_stats(int* rounds, int* jumps, int capacity);

/* ---- density clustering (Old/StatisticalOutlierRemoval.py: remove_outliers_keep_color2) ----
 * compute_nearest_neighbor_distance, cluster_dbscan and remove_radius_outlier
 * restated (csrc/slcluster.inl; tests/cluster_oracle.py is the CPU restatement,
 * exact; parity with Open3D unpinned).  xyz [n][3]: device f64.
 *   neighbourhood  j is a neighbour of i iff ((dx dx + dy dy) + dz dz) < r r in
 *                  f64, uncontracted, in that order; i itself is one.
 * sl_radius_count: min(neighbour count, cap) of every point -> out_cnt [n]
 * (device int32); cap <= 0: the exact count.  remove_radius_outlier(nb_points,
 * radius) keeps the points with a count > nb_points (cap nb_points + 1).
 * sl_cluster_dbscan: PointCloud::ClusterDBSCAN's labels in their order-free
 * form -> labels [n] (device int32), the number of clusters -> *n_clusters
 * (host, may be NULL):
 *   core     neighbour count >= min_points;
 *   cluster  a connected component of the core points (edges: neighbours);
 *   label    the rank of the cluster's smallest core index among the clusters'
 *            smallest core indices, 0, 1, 2, ...;
 *   border   a non-core point with a core neighbour: the smallest label among
 *            its core neighbours' clusters;
 *   noise    a non-core point without a core neighbour: -1.
 * Lock-free union-find on the device (roots hooked under smaller roots by
 * compare-and-swap); nothing spins and the host iterates nothing.  Scratch: the
 * search grid + 28 n bytes.  sl_cluster_dbscan_stats: the calling thread's last
 * call's host milliseconds per stage (grid, count, union, flatten + rank,
 * border; stage_ms[capacity], zero-filled) -- a measurement aid.
 * sl_nearest_neighbor_distance: the distance to the nearest other point (the
 * second entry of the exact 2-NN, ties by (d2, index): a duplicated point gives
 * 0) -> out [n] (device f64); 0 for n == 1.
 * All: n == 0 succeeds and writes nothing.  SL_EINVAL with a message: NULL
 * arguments, n >= 2^31, non-finite coordinates, radius / eps <= 0 or not
 * finite, min_points < 1.  Blocking on `stream`. */
int sl_radius_count(sl_ctx* ctx, const double* xyz, int64_t n, double radius, int cap, int32_t* out_cnt,
                    void* stream);
int sl_cluster_dbscan(sl_ctx* ctx, const double* xyz, int64_t n, double eps, int min_points, int32_t* labels,
                      int64_t* n_clusters, void* stream);
int sl_cluster_dbscan_stats(double* stage_ms, int capacity);
int sl_nearest_neighbor_distance(sl_ctx* ctx, const double* xyz, int64_t n, double* out, void* stream);

/* ---- ball-pivoting surface meshing (csrc/slbpa.inl) ----
 * The reference's reconstruct_stl(mode="surface") (server/processing.py:220-237)
 * is Open3D's create_from_point_cloud_ball_pivoting, restated in an order-free
 * form (slbpa.inl states the rules; tests/bpa_oracle.py is their CPU form).
 * sl_ball_pivot_candidates: the triangles (i, j, k) of the cloud that have an
 * empty ball of `radius` on the side of their three normals, among the points
 * that are not inner (vclass u8 [n]: 0 orphan, 1 border, 2 inner; NULL: all
 * orphans) -> triangles int32 [capacity][3] (device), wound so that the face
 * normal is on the ball's side, in the lexicographic order of their sorted
 * triples (two runs write identical arrays), and *count (host).  When *count
 * exceeds `capacity` nothing is written: call again with capacity >= *count.
 * A point with more than sl_ball_pivot_max_neighbours() points within twice
 * the radius (itself included) is SL_EINVAL with a message naming the count
 * and the limit; a neighbourhood is never truncated.  n == 0 succeeds.
 * SL_EINVAL with a message: NULL arguments, n >= 2^31, non-finite coordinates,
 * a radius that is not finite and positive.  Blocking on `stream`.
 * sl_ball_pivot_candidates_stats: of this thread's last call, host
 * milliseconds of the grid, the enumeration and the ordering, then the live
 * queries, the candidates, the neighbourhood that was too large and the
 * queries of the kernel's second tier (stats[capacity], zero-filled) -- a
 * measurement aid. */
int sl_ball_pivot_max_neighbours(void);
int sl_ball_pivot_candidates(sl_ctx* ctx, const double* xyz, const double* normals, int64_t n, double radius,
                             const uint8_t* vclass, int32_t* triangles, int64_t capacity, int64_t* count,
                             void* stream);
int sl_ball_pivot_candidates_stats(double* stats, int capacity);

/* Release the scratch buffers the merge entry points keep pooled for `device`
 * (kept otherwise for the process's lifetime, at most 16 GiB per device);
 * the bytes released -> *released_bytes (may be NULL). */
int sl_merge_pool_trim(int device, int64_t* released_bytes);

/* Test aid: poison the merge pool's scratch.  byte 0..255 arms the mode: every
 * buffer the pool hands out from then on (reused or fresh) has the bytes that
 * were asked for filled with that value, on the stream of the entry point
 * that asked, before that entry point's first kernel; -1 disarms it (the
 * default); anything else is SL_EINVAL and changes nothing.  The bytes
 * filled so far in this process, never reset -> *poisoned_bytes (may be NULL).
 * Results must not depend on the mode: a difference is a word read before it
 * is written.  The context-owned scratch of the decode path and of the PLY
 * reader and writer is not pooled and not covered. */
int sl_merge_pool_poison(int byte, int64_t* poisoned_bytes);

/* ---- multi-GPU gather ----
 * The merge's one exchange: every rank's cloud to `root` in rank order over
 * RCCL (opened with dlopen by soname, so a process that already holds
 * PyTorch's RCCL shares that copy).  One context per rank (GPU):
 *   sl_gather_unique_id  one rank makes the 128-byte id, shared out of band
 *                        (the Python side uses torch.distributed.broadcast_object_list);
 *   sl_gather_init       ncclCommInitRank on the context's device;
 *   sl_gather_counts     blocking: an ncclAllGather of one int64 per rank ->
 *                        counts_out[nranks] (host) on every rank, so the root
 *                        can size its buffers;
 *   sl_gather            grouped ncclSend / ncclRecv of xyz (f32 or f64, 3 per
 *                        point) and bgr (3 B per point) into the root's
 *                        xyz_out / bgr_out at exclusive-scan offsets of
 *                        `counts`; asynchronous on `stream`.
 * Replaces the sequential per-file merge of processing.py:116-140. */
int sl_gather_unique_id(uint8_t* id_out /* 128 bytes */);
int sl_gather_init(sl_ctx* ctx, int nranks, int rank, const uint8_t* id /* 128 bytes */);
int sl_gather_counts(sl_ctx* ctx, int64_t n_local, int64_t* counts_out, void* stream);
int sl_gather(sl_ctx* ctx, const void* xyz, int xyz_dtype, const uint8_t* bgr, const int64_t* counts, int root,
              void* xyz_out, uint8_t* bgr_out, void* stream);

/* The names of SURVEY.md §8(b): sl_decode_triangulate is already batched (V
 * views per call); sl_last_error is sl_ctx_last_error. */
int sl_decode_triangulate_batch(sl_ctx* ctx, const uint8_t* stack, int64_t stack_view_stride, int n_views,
                                int n_img, int H, int W, int n_cols, int n_rows, const uint8_t* tex_bgr,
                                int64_t tex_view_stride, int mask_mode, const double* poses, int32_t* col_out,
                                int32_t* row_out, uint8_t* mask_out, void* xyz_out, int xyz_dtype,
                                uint8_t* bgr_out, int64_t out_capacity, int64_t* view_offsets, void* stream);
const char* sl_last_error(const sl_ctx* ctx);

/* ---- calibration products (csrc/slcalib.hip) ----
 * Replaces the NumPy tail of SLSystem.calibrate_final (server/sl_system.py:348-403):
 * from the stereo parameters OpenCV estimated (cam_K = K1, proj_K = K2, R, T;
 * row-major 3x3 / 3) it derives, on the device,
 *   nc_out        [3][cam_h*cam_w]  unit camera rays, pixel v*cam_w + u (Nc, :353-365)
 *   plane_col_out [4][proj_w]       column planes (n0, n1, n2, d) (wPlaneCol as saved, :397-398, :408)
 *   plane_row_out [4][proj_h]       row planes (wPlaneRow, :401-402, :409)
 * (any output may be NULL; proj_w x proj_h = SCREEN_WIDTH x SCREEN_HEIGHT of
 * config.py).  Bit-identical to the reference's NumPy 2.2 / OpenBLAS 0.3.29
 * evaluation (3-term dots as left-to-right FMA chains).  Asynchronous. */
int sl_calib_products(sl_ctx* ctx, const double* cam_K, const double* proj_K, const double* R, const double* T,
                      int cam_w, int cam_h, int proj_w, int proj_h, double* nc_out, double* plane_col_out,
                      double* plane_row_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLGPU_H */
