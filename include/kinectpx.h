/*
 * kinectpx.h -- C ABI of libkinectpx.so: the MI355X (gfx950) hot path behind KinectPy's
 * preprocessing.{extractor,filtering,registration} and floor_removal module APIs.
 *
 * The reference (tiborcamargo/KinectPy) is pure Python: it has no FFI layer; its "operators" are
 * module functions that call Open3D.  Each entry point below names the reference interface it
 * replaces (file:line under the reference root) -- the ctypes stubs a maintainer would add are in
 * INTEGRATION.md.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name starts with `h_`; the caller owns all memory
 *    (torch-ROCm tensors in the Python host); the library never allocates user-visible memory;
 *  - scratch comes from a caller-provided workspace `ws` of at least `kpx_*_workspace_bytes()` bytes,
 *    256-byte aligned;
 *  - clouds are float32 (N,3) row-major ("xyz xyz ..."), colours/normals likewise; index arrays are
 *    int32; rigid transforms are float64 row-major 4x4 (the reference's .npy interchange format,
 *    preprocessing/data.py:158-160);
 *  - outputs of data-dependent length are written into worst-case-sized buffers and their length
 *    into a device int32 (`d_count`);
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream)
 *    and returns 0 or a negative kpx_status; `kpx_last_error()` (thread-local) has the message;
 *  - no C++ exception crosses this boundary.
 */
#ifndef KINECTPX_H
#define KINECTPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPX_VERSION 100

typedef enum {
    KPX_OK = 0,
    KPX_ERR_INVALID = -1,     /* invalid argument (Open3D raises RuntimeError / ValueError here) */
    KPX_ERR_WORKSPACE = -2,   /* workspace too small */
    KPX_ERR_RANGE = -3,       /* value out of the supported range (e.g. voxel index overflow) */
    KPX_ERR_HIP = -4,         /* a HIP runtime call failed */
    KPX_RETRY = 1             /* kpx_frame_step_sharded: a message outgrew its capacity on every rank alike; run the frame again */
} kpx_status;

const char *kpx_last_error(void);
int kpx_version(void);

/* ---- extract stage -------------------------------------------------------------------------- */

/* a1: depth -> XYZ int16 millimetres, the `<ts>_depth.dat` layout that utils/io.py:15-20
 * (load_depth) reads and that preprocessing/extractor.py:68-80 obtains from an external binary.
 * xyz[i] = (floorf(xt*d+0.5f), floorf(yt*d+0.5f), d), (0,0,0) when d==0 or the table entry is NaN.
 * depth: u16 [frames*n_px]; xy_table: f32 [n_px*2] shared by all frames; xyz: i16 [frames*n_px*3]. */
int kpx_unproject_u16(const uint16_t *depth, const float *xy_table, int64_t n_px, int32_t frames,
                      int16_t *xyz, void *stream);

/* a4: np.median of the z column (preprocessing/data.py:170-171), exact, per frame.
 * v: i16 values with `stride` elements between consecutive samples (3 for the z column of an
 * (N,3) .dat array, 1 for a raw depth frame); d_median: f64 [frames]. */
size_t kpx_median_workspace_bytes(int32_t frames);
int kpx_median_i16(const int16_t *v, int64_t n, int64_t stride, int32_t frames, double *d_median,
                   void *ws, size_t ws_bytes, void *stream);

/* a3 + a4: utils/io.py:23-43 rgbd_to_pointcloud (keep = x!=0 & y!=0 & z!=0, colours/255) composed
 * with preprocessing/data.py:165-178 (_transform_filtered_image_to_pointcloud: all colour
 * channels != 0, z <= median + gate).  Order-preserving compaction, per frame.
 * rgb may be NULL (no colours, no colour mask).  flags: bit0 = colour mask, bit1 = depth gate
 * (needs d_median).  Outputs per frame f at offset f*n: pts f32 [n*3], col f32 [n*3] (optional),
 * idx i32 [n] (optional, source pixel index), d_count i32 [frames]. */
#define KPX_COMPACT_COLOR_MASK 1
#define KPX_COMPACT_DEPTH_GATE 2
size_t kpx_compact_workspace_bytes(int64_t n, int32_t frames);
int kpx_rgbd_compact(const int16_t *xyz, const uint8_t *rgb, int64_t n, int32_t frames, int32_t flags,
                     const double *d_median, double gate, float *pts, float *col, int32_t *idx,
                     int32_t *d_count, void *ws, size_t ws_bytes, void *stream);

/* Fused a1+a3+a4 for the streaming pipeline: u16 depth (+ xy table, + optional rgb) straight to the
 * compacted float32 cloud, never materialising the int16 XYZ image.  Same outputs as
 * kpx_rgbd_compact; the median is taken over the raw depth (== the z column).
 * Both entries take at most as many frames per call as the device's grid has rows (hipDeviceAttributeMaxGridDimY: 65536 on the
 * MI355X) and return KPX_ERR_INVALID for more. */
size_t kpx_depth_to_cloud_workspace_bytes(int64_t n_px, int32_t frames);
int kpx_depth_to_cloud(const uint16_t *depth, const float *xy_table, const uint8_t *rgb, int64_t n_px,
                       int32_t frames, int32_t flags, double gate, float *pts, float *col, int32_t *idx,
                       int32_t *d_count, void *ws, size_t ws_bytes, void *stream);

/* ---- container operations (Open3D surface used by the path) ------------------ */

/* a17: pcd.transform(T) (preprocessing/data.py:48) -- out = R p + t (fp64 fma chain, stored f32).
 * normals (optional, in place rotation only).  in == out allowed. */
int kpx_transform(const float *pts, int64_t n, const double *h_T, float *out, void *stream);
int kpx_rotate(const float *nrm, int64_t n, const double *h_T, float *out, void *stream);
/* a5: align_skeletons / transform_joints (preprocessing/extractor.py:113-116,
 * utils/processing.py:357-383): out = x @ inv(R) + t on f64 (rows,3) joints; h_A = inv(R) row-major 3x3. */
int kpx_joints_affine_f64(const double *x, int64_t rows, const double *h_A, const double *h_t, double *out,
                          void *stream);

/* select_by_index (floor_removal.py:50,69,71,72): selection of up to three (n,3) f32 attributes.
 * [O3D] SelectByIndex marks the listed points in a mask and emits the marked (or, inverted, the unmarked) points in
 * ascending original order: duplicates collapse, the order of the list does not matter.
 * KPX_SELECT_GATHER (0): out[k] = in[idx[k]] for k < n_idx -- equal to Open3D for ascending duplicate-free lists (the
 *                        keep lists / inlier lists this library produces, np.argwhere results), one gather, no count;
 * KPX_SELECT_INVERT (1): ascending complement of idx; d_count receives its length;
 * KPX_SELECT_MASK   (2): the mask semantics for arbitrary lists (unsorted, repeated); d_count receives the length.
 * Modes 1 and 2 need a workspace of kpx_select_workspace_bytes(n); mode 0 needs none (ws may be NULL). */
#define KPX_SELECT_GATHER 0
#define KPX_SELECT_INVERT 1
#define KPX_SELECT_MASK 2
size_t kpx_select_workspace_bytes(int64_t n);
int kpx_select_by_index(const float *a0, const float *a1, const float *a2, int64_t n, const int32_t *idx,
                        int64_t n_idx, int32_t invert, float *o0, float *o1, float *o2, int32_t *d_count,
                        void *ws, size_t ws_bytes, void *stream);

/* The same gather (KPX_SELECT_GATHER) that also leaves the bounds of the points it wrote -- min x, y, z, max x, y, z as six doubles at
 * d_bbox6 -- so that the selected cloud's next consumer (kpx_slab_split_bounded: floor_removal.py:64-66 takes max(y) of the cloud it just
 * filtered) needs no pass of its own for them.  n_idx > 0; workspace: kpx_select_workspace_bytes(n). */
int kpx_select_by_index_bounds(const float *a0, const float *a1, const float *a2, int64_t n, const int32_t *idx, int64_t n_idx,
                               float *o0, float *o1, float *o2, double *d_bbox6, void *ws, size_t ws_bytes, void *stream);
/* Open3D get_min_bound / get_max_bound, numpy's pcd_points[:, 1].max() (floor_removal.py:65-66): min x, y, z, max x, y, z of an
 * (n,3) f32 cloud as six doubles in device memory.  n > 0. */
size_t kpx_bounds_workspace_bytes(void);
int kpx_bounds(const float *pts, int64_t n, double *d_bbox6, void *ws, size_t ws_bytes, void *stream);

/* Stable sort of (key, value) pairs by the low end_bit (1..32) bits of the key -- the ordering step behind a7 / a8 / a11 (voxel keys,
 * grid cells, Morton codes; the reference gets it from Open3D's hash maps and np.argsort).  Inputs are not modified and may not
 * alias the outputs. */
size_t kpx_sort_pairs_u32_workspace_bytes(int64_t n);
int kpx_sort_pairs_u32(const uint32_t *keys_in, const int32_t *vals_in, int64_t n, int32_t end_bit, uint32_t *keys_out,
                       int32_t *vals_out, void *ws, size_t ws_bytes, void *stream);

/* a19: pcd_above_plane (floor_removal.py:39-51): indices of points with a x + b y + c z + d < 0
 * (evaluated left to right in fp64, as the reference's Python loop). */
int kpx_halfspace_select(const float *pts, int64_t n, const double *h_plane, int32_t *idx, int32_t *d_count,
                         void *ws, size_t ws_bytes, void *stream);
/* floor_removal.py:64-66: y >= max(y) - slab  -> lower indices, y < max(y) - slab -> upper indices. */
int kpx_slab_split(const float *pts, int64_t n, double slab, int32_t *lower_idx, int32_t *d_lower,
                   int32_t *upper_idx, int32_t *d_upper, void *ws, size_t ws_bytes, void *stream);
/* The same split for a cloud whose bounds are already in device memory (d_bbox6 as written by kpx_bounds or
 * kpx_select_by_index_bounds; only max y, d_bbox6[4], is read): one pass over the points instead of two. */
int kpx_slab_split_bounded(const float *pts, int64_t n, double slab, const double *d_bbox6, int32_t *lower_idx, int32_t *d_lower,
                           int32_t *upper_idx, int32_t *d_upper, void *ws, size_t ws_bytes, void *stream);

/* ---- filter stage ------------------------------------------------------------------------------ */

/* a7: PointCloud.voxel_down_sample(v) (preprocessing/filtering.py:23, registration.py:8,100,101).
 * origin = min_bound - v/2, index = floor((p-origin)/v), per-voxel mean of points / colours /
 * normals (normals renormalised).  Output order: ascending (ix,iy,iz) (documented deviation from
 * Open3D's hash order).  col/nrm and their outputs may be NULL. */
size_t kpx_voxel_workspace_bytes(int64_t n);
int kpx_voxel_downsample(const float *pts, const float *col, const float *nrm, int64_t n, double voxel,
                         float *opts, float *ocol, float *onrm, int32_t *d_count, void *ws, size_t ws_bytes,
                         void *stream);

/* The same for `count` independent clouds (the per-device clouds of one frame set, preprocessing/data.py:129-143 /
 * registration.py:24-29 down-sample every device's cloud): the clouds are processed side by side on internal
 * lanes; `stream` continues after all of them.  h_*: host arrays of device pointers (h_col / h_ocol may be NULL),
 * d_counts: i32 [count] on the device. */
size_t kpx_voxel_batch_workspace_bytes(int32_t count, const int64_t *h_n);
int kpx_voxel_downsample_batch(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n,
                               double voxel, float *const *h_opts, float *const *h_ocol, int32_t *d_counts, void *ws,
                               size_t ws_bytes, void *stream);

/* a17 + a7 in one pass -- the fuse of the frame loop, preprocessing/data.py:44-61: cloud c is moved by its registration
 * h_T[c] (pcd.transform(T), :48; 4x4 row-major f64 on the host, identity for the master), the clouds are stacked in the given
 * order (np.vstack, :55-58) and the stack is voxel_down_sample'd (filter_outliers, filtering.py:23).  The stacked cloud is
 * never materialised: the reference holds it in float64, so the minimum bound, the voxel index and the per-voxel sums use the
 * fp64 value of the moved point recomputed from the float32 sensor point -- voxel membership is the float64 path's, which a
 * float32 copy of the moved points does not guarantee.  Up to 16 clouds; h_col (and ocol) may be NULL; colours must be on all
 * non-empty clouds or on none.  opts / ocol: f32 [sum n][3] worst case; d_count = voxels.  Output order as kpx_voxel_downsample. */
size_t kpx_fuse_voxel_workspace_bytes(int64_t total_points);
int kpx_fuse_voxel_downsample(int32_t count, const float *const *h_pts, const float *const *h_col, const int64_t *h_n,
                              const double *h_T, double voxel, float *opts, float *ocol, int32_t *d_count, void *ws,
                              size_t ws_bytes, void *stream);

/* a8: PointCloud.remove_statistical_outlier(nb_neighbors, std_ratio) (filtering.py:24,
 * floor_removal.py:73, utils/processing.py:309).  keep_idx ascending, d_count = kept,
 * d_stats f64 [3] = (mean, std, threshold), d_avg f64 [n] (optional) = per-point mean kNN distance.
 * nb_neighbors <= KPX_SOR_MAX_K.  Up to KPX_SOR_LDS_K the neighbour heaps of the queries the wave passes leave over live in LDS;
 * beyond, in the workspace (global memory: slower, the same result) -- the reference takes any value (preprocessing/filtering.py:12-17). */
#define KPX_SOR_MAX_K 4096
#define KPX_SOR_LDS_K 288
size_t kpx_sor_workspace_bytes(int64_t n, int32_t nb_neighbors);
int kpx_sor(const float *pts, int64_t n, int32_t nb_neighbors, double std_ratio, int32_t *keep_idx,
            int32_t *d_count, double *d_stats, double *d_avg, void *ws, size_t ws_bytes, void *stream);

/* `cl, ind = pcd.remove_statistical_outlier(nb_neighbors, std_ratio)` (preprocessing/filtering.py:33, data.py:61) with BOTH results:
 * the keep list as kpx_sor and, in the same pass, the kept rows of pts (and of one more (n,3) attribute array, e.g. colours; NULL for
 * none) -- kpx_sor + kpx_select_by_index without the count read-back in between.  Workspace: kpx_sor_workspace_bytes. */
int kpx_sor_select(const float *pts, const float *attr, int64_t n, int32_t nb_neighbors, double std_ratio, float *out_pts,
                   float *out_attr, int32_t *keep_idx, int32_t *d_count, double *d_stats, void *ws, size_t ws_bytes, void *stream);

/* The same filter sharded over GPUs (the fused-cloud filter_outliers of preprocessing/data.py:61 when every GPU holds the
 * fused cloud): the grid order of the cloud is the same on every GPU, each searches only the queries at
 * cell-sorted positions [q_begin, q_end) -- a spatial slab -- and writes their mean distances, in that order, to
 * d_avg_sorted f64 [q_end - q_begin]; d_order i32 [n] (optional) receives the cell-sorted position -> point index map.
 * After the slabs have been exchanged (one all-gather), kpx_sor_finish(avg of all n positions, d_order) computes mean / std /
 * threshold and the ascending keep list with the same kernels and the same reduction order as kpx_sor: the result is
 * bit-identical to the one-GPU call.  Workspace of kpx_sor_partial: kpx_sor_workspace_bytes(n, nb_neighbors). */
int kpx_sor_partial(const float *pts, int64_t n, int32_t nb_neighbors, int64_t q_begin, int64_t q_end, double *d_avg_sorted,
                    int32_t *d_order, void *ws, size_t ws_bytes, void *stream);
size_t kpx_sor_finish_workspace_bytes(int64_t n);
int kpx_sor_finish(const double *d_avg_sorted, const int32_t *d_order, int64_t n, double std_ratio, int32_t *keep_idx,
                   int32_t *d_count, double *d_stats, double *d_avg, void *ws, size_t ws_bytes, void *stream);

/* labels = pcd.cluster_dbscan(eps, min_points) ([O3D] PointCloud::ClusterDBSCAN; the geometric stand-in for the person mask of
 * preprocessing/filtering.py:28-95).  Neighbours: every point (itself included) with d2 < eps^2 (AC3, strict <).  A point is core
 * iff it has >= min_points neighbours (0 or 1: every point); clusters are the connected components of the core points, numbered
 * by their smallest core index; a non-core point takes the smallest id among its core neighbours, or -1 -- exactly the labels of
 * Open3D's sequential loop, bit-identical run to run.  labels i32 [n]; d_nclusters = number of clusters (a negative kpx_status if
 * the union pass gave up).  Rejects !(eps > 0) and min_points < 0.  n == 0: d_nclusters = 0. */
size_t kpx_dbscan_workspace_bytes(int64_t n);
int kpx_cluster_dbscan(const float *pts, int64_t n, double eps, int32_t min_points, int32_t *labels /* [n] */,
                       int32_t *d_nclusters, void *ws, size_t ws_bytes, void *stream);

/* cl, ind = pcd.remove_radius_outlier(nb_points, radius) ([O3D] PointCloud::RemoveRadiusOutliers): point i is kept iff it has
 * more than nb_points neighbours with d2 < radius^2 (itself included; AC3, strict <).  keep_idx ascending, d_count = kept.
 * Rejects nb_points < 1 or !(radius > 0) with Open3D's message. */
size_t kpx_radius_outlier_workspace_bytes(int64_t n);
int kpx_remove_radius_outlier(const float *pts, int64_t n, int32_t nb_points, double radius, int32_t *keep_idx,
                              int32_t *d_count, void *ws, size_t ws_bytes, void *stream);

/* keypoints = o3d.geometry.keypoint.compute_iss_keypoints(pcd, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
 * ([O3D] geometry::keypoint::ComputeISSKeypoints, Zhong 2009).  Neighbours of i within r: every j (i included) with d2 < r^2 (AC3,
 * strict <).  Saliency s_i: with m = #neighbours within salient_radius, s_i = 0 if m < min_neighbors; else C = covariance of those
 * points in Open3D's raw-moment form (nine moments / m, C_ab = E[ab] - E[a] E[b]; fp64), s_i = 0 if every |C_ab| <= 1e-12; else with
 * the eigenvalues e3 <= e2 <= e1 of C, s_i = e3 if e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (a NaN ratio fails), else 0.
 * i is a keypoint iff s_i > 0, it has >= min_neighbors neighbours within non_max_radius and none of them has a larger saliency
 * (equal saliencies do not suppress each other).  keep_idx ascending, d_count = keypoints.
 *   kpx_iss_saliency  writes saliency f64 [n] (by point index);
 *   kpx_iss_nonmax    suppresses ANY caller-supplied saliency f64 [n] (NaN, zero and negative entries are never keypoints);
 *   kpx_iss_keypoints both on one grid: saliency [n] out, keep_idx [n], d_count.
 * The radii are given (the defaults of Open3D's 0.0 -- 6 x and 4 x the mean nearest-neighbour distance -- are resolved by the caller,
 * kpx_mean_nn_distance).  Rejects radii that are not positive and finite and min_neighbors < 0.  n == 0: d_count = 0. */
size_t kpx_iss_workspace_bytes(int64_t n);
int kpx_iss_saliency(const float *pts, int64_t n, double salient_radius, double gamma_21, double gamma_32, int32_t min_neighbors,
                     double *saliency /* [n] */, void *ws, size_t ws_bytes, void *stream);
int kpx_iss_nonmax(const float *pts, int64_t n, const double *saliency /* [n] */, double non_max_radius, int32_t min_neighbors,
                   int32_t *keep_idx, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_iss_keypoints(const float *pts, int64_t n, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                      int32_t min_neighbors, double *saliency /* [n] */, int32_t *keep_idx, int32_t *d_count, void *ws, size_t ws_bytes,
                      void *stream);
/* Mean of [O3D] ComputeNearestNeighborDistance from a 2-nearest search of a cloud on itself (kpx_search_knn, k = 2): d_mean =
 * (sum over rows with count >= 2 of sqrt(d2[row * stride + 1])) / m, the sum exact in 128-bit fixed point -- the same bits whatever
 * the order of the adds.  ws: 256 bytes. */
int kpx_mean_nn_distance(const double *d2, const int32_t *count, int64_t m, int32_t stride, double *d_mean, void *ws, size_t ws_bytes,
                         void *stream);

/* pcd.farthest_point_down_sample(k, start_index) ([O3D] PointCloud::FarthestPointDownSample): the fixed-size input of the PointNet
 * regressor (datasets/kinect_dataset*.py, number_of_points) by farthest-point sampling instead of a uniform draw.  Open3D's loop:
 *   dist[j] = +inf; far = start_index; for i < k: sel[i] = far; s = p[far]; max_dist = 0;
 *     for j ascending: dist[j] = min(dist[j], d2(p[j], s)); if (dist[j] > max_dist) { max_dist = dist[j]; far = j; }
 * d2 = AC3 in fp64 of the float32 coordinates (equal to Open3D's (dx^2 + dy^2) + dz^2 whenever every square is exact, e.g. integer
 * millimetres).  So sample i + 1 is the smallest index among the points of largest dist, and when every dist is 0 (only duplicates
 * left) the previous index repeats.  sel i32 [k] in selection order, repeats kept (Open3D's selected_indices; the down-sampled cloud
 * is SelectByIndex(sel), mask semantics); cover f64 [k] (nullable) = max_dist of iteration i, the squared coverage radius after
 * i + 1 samples (non-increasing).  Bit-identical run to run and across forms.  Rejects k > n ("Illegal number of samples") and, for
 * k > 0, start_index >= n ("Illegal start index"); k == 0 writes nothing.  (Open3D returns a copy for k == n without the loop; the
 * ABI runs it.)  Non-finite coordinates are outside the contract.
 * Forms: one block of KPX_FPS_BLOCK_THREADS threads per cloud (block form; all such clouds of a batch in one launch, one barrier
 * per sample; a point's running dist stays in registers for the first KPX_FPS_REG_N points, in LDS up to KPX_FPS_LDS_N, in the
 * workspace beyond), or a chain of k + 1 launches over the whole device (each reduces the previous launch's per-block candidates,
 * then updates its slice of dist).  Dispatch, from measurement (MI355X): the chain costs ~5.6 us per sample at any
 * size, the block form 2.5 us at 8k points, 4.0 at 19k and ~0.33 us more per 1000 points beyond.  A cloud takes the block form
 * when n <= KPX_FPS_BLOCK_MAX_N; in a batch with at least KPX_FPS_BATCH_MIN_CLOUDS clouds of KPX_FPS_BLOCK_MAX_N < n <=
 * KPX_FPS_BATCH_BLOCK_MAX_N, those join the block launch too (they run side by side, while chains run one after another).
 * Batch: h_* are host arrays of device pointers (h_cover may be NULL, or hold NULL entries); k and start_index hold for every
 * cloud.  Workspace: kpx_fps_workspace_bytes(count, max n). */
#define KPX_FPS_BLOCK_THREADS 1024
#define KPX_FPS_REG_N 12288
#define KPX_FPS_LDS_N 19456
#define KPX_FPS_BLOCK_MAX_N 24576
#define KPX_FPS_BATCH_BLOCK_MAX_N 65536
#define KPX_FPS_BATCH_MIN_CLOUDS 4
size_t kpx_fps_workspace_bytes(int32_t count, int64_t n_max);
int kpx_farthest_point_sample(const float *pts, int64_t n, int32_t k, int32_t start_index, int32_t *sel /* [k] */,
                              double *cover /* [k] or NULL */, void *ws, size_t ws_bytes, void *stream);
int kpx_farthest_point_sample_batch(int32_t count, const float *const *h_pts, const int64_t *h_n, int32_t k, int32_t start_index,
                                    int32_t *const *h_sel, double *const *h_cover, void *ws, size_t ws_bytes, void *stream);

/* estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) (preprocessing/registration.py:9-13):
 * neighbours = up to max_nn nearest with d2 < radius^2; < 3 neighbours -> (0,0,1); else the
 * eigenvector of the smallest eigenvalue of the neighbourhood covariance.  max_nn <= KPX_NORMALS_MAX_NN (beyond KPX_NORMALS_LDS_NN the
 * fall-back heaps live in the workspace instead of LDS; preprocessing/registration.py:7-21 takes any value). */
#define KPX_NORMALS_MAX_NN 4096
#define KPX_NORMALS_LDS_NN 128
size_t kpx_normals_workspace_bytes(int64_t n, int32_t max_nn);
int kpx_estimate_normals(const float *pts, int64_t n, double radius, int32_t max_nn, float *normals,
                         void *ws, size_t ws_bytes, void *stream);
/* PointCloud.estimate_covariances(search_param): per point the covariance of the estimate_normals neighbourhood (same search,
 * same ties), E[x x^T] - mu mu^T with divisor m; < 3 neighbours -> the identity.  cov f64 [n][9] (symmetric, row-major). */
size_t kpx_covariances_workspace_bytes(int64_t n, int32_t max_nn);
int kpx_estimate_covariances(const float *pts, int64_t n, double radius, int32_t max_nn, double *cov,
                             void *ws, size_t ws_bytes, void *stream);

/* Self-test of the whole-wave primitives the neighbour searches reduce, scan and broadcast with (csrc/kpx_wave.h): one block of four
 * waves, every wave applies primitive `kind` to rows of 64 values.  in / out: u64 [rows][64] in device memory, the 32-bit kinds use
 * the low word; out[r][l] is what lane l holds afterwards (the SUM_DOWN kinds define lane 0 only; F64X9 reduces groups of nine rows
 * together and stores lane 0, rows % 9 == 0; BCAST broadcasts lane r % 64 of row r).  rows <= 65536. */
#define KPX_WAVE_SUM_I32 0
#define KPX_WAVE_MIN_U32 1
#define KPX_WAVE_MAX_U32 2
#define KPX_WAVE_MAX_U64 3
#define KPX_WAVE_MAX_F64 4
#define KPX_WAVE_INCL_SCAN_I32 5
#define KPX_WAVE_BCAST 6
#define KPX_WAVE_SUM_DOWN_F64 7
#define KPX_WAVE_SUM_DOWN_F32 8
#define KPX_WAVE_SUM_DOWN_F64X9 9
int kpx_wave_selftest(int32_t kind, const uint64_t *in, int64_t rows, uint64_t *out, void *stream);

/* The group pass of the neighbour search (four queries per wave, in front of the wave-per-query passes of kpx_sor* with nb_neighbors
 * <= 32 and of kpx_estimate_normals / kpx_estimate_covariances with max_nn <= 48): out[0] = the queries the calling thread's last such
 * pass was given, out[1] = the ones it handed on to the passes behind it; {0, 0} before any.  Read back from the pass's counter word in
 * that call's workspace -- valid until the workspace is used again -- after a synchronisation of that call's stream.  For tests and
 * measurements: no result depends on which pass settled a query. */
int kpx_knn_group_last(int64_t *out /* [2] */);

/* Neighbour search between a cloud and ARBITRARY query points ([O3D] KDTreeFlann SearchKNN / SearchRadius / SearchHybrid).
 * The index is a caller-owned device buffer of kpx_search_index_bytes(n) bytes that kpx_search_index_build fills from a float32 (n,3)
 * cloud: grid parameters, cell starts, cell-sorted coordinates, original indices.  It does not point back into pts and the library keeps
 * no state: it may be queried any number of times, copied, and outlives the cloud.  n == 0 and degenerate bounding boxes are fine.
 * Queries are float32 (m,3).  d2 = AC3 in fp64 (d = q - p); every result row ascends in (d2, index) -- on equal d2 the LOWEST cloud index
 * comes first (Open3D leaves the order of ties open).  A query with a non-finite coordinate finds nothing; results do not depend on the
 * grid, the launch shape or the order of the queries.
 *   kpx_search_knn: radius <= 0: the min(k, n) nearest; radius > 0: hybrid, the first min(k, count) of the radius result.  idx i32 [m][k],
 *     d2 f64 [m][k], count i32 [m]; slots past count hold -1 / +inf.  1 <= k <= 4096.
 *   kpx_search_radius_count: offsets i64 [m+1] = exclusive scan of the per-query number of points with d2 < radius*radius (strict, r2 in
 *     fp64), offsets[m] = total.  The caller reads the total, allocates idx i32 [total] and d2 f64 [total], and calls
 *   kpx_search_radius_fill with the same index, queries, radius and offsets: segment q = [offsets[q], offsets[q+1]) sorted.  A total above
 *     2^31 - 1 is KPX_ERR_RANGE.  Both reject !(radius > 0).
 * Every query call reads the index header back (one small copy and a synchronisation of `stream`) and rejects a buffer that is not
 * an index or whose index_bytes is smaller than kpx_search_index_bytes of the n it records; k, radius, a null index and an
 * index_bytes below kpx_search_index_bytes(0) are rejected before the device is touched.
 * Workspace: kpx_search_workspace_bytes(m, k) for the three query calls (m queries); kpx_search_workspace_bytes(n, 0) for
 * kpx_search_index_build of an n-point cloud. */
size_t kpx_search_index_bytes(int64_t n);
int kpx_search_index_build(const float *pts, int64_t n, void *index, size_t index_bytes, void *ws, size_t ws_bytes, void *stream);
size_t kpx_search_workspace_bytes(int64_t m, int32_t k);
int kpx_search_knn(const void *index, size_t index_bytes, const float *queries, int64_t m, int32_t k, double radius, int32_t *idx /* [m][k] */,
                   double *d2 /* [m][k] */, int32_t *count /* [m] */, void *ws, size_t ws_bytes, void *stream);
int kpx_search_radius_count(const void *index, size_t index_bytes, const float *queries, int64_t m, double radius, int64_t *offsets /* [m+1] */,
                            void *ws, size_t ws_bytes, void *stream);
int kpx_search_radius_fill(const void *index, size_t index_bytes, const float *queries, int64_t m, double radius, const int64_t *offsets,
                           int64_t total, int32_t *idx /* [total] */, double *d2 /* [total] */, void *ws, size_t ws_bytes, void *stream);

/* a21: PointCloud.segment_plane(distance_threshold, ransac_n, num_iterations) (floor_removal.py:70).
 * Seeded (Philox4x32-10) so results are reproducible; the reference's is unseeded.
 * d_plane f64 [4], inlier_idx ascending, d_count = #inliers. */
size_t kpx_segment_plane_workspace_bytes(int64_t n, int32_t ransac_n, int32_t num_iterations);
int kpx_segment_plane(const float *pts, int64_t n, double distance_threshold, int32_t ransac_n,
                      int32_t num_iterations, double probability, uint64_t seed, double *d_plane,
                      int32_t *inlier_idx, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);

/* ---- register stage ---------------------------------------------------------------------------- */

/* One correspondence search of registration_icp (manual_pointcloud_registration.py:96-98,
 * preprocessing/registration.py:78-84): for every source point transformed by d_T (device f64 [16]),
 * the nearest target point (exact; ties to the lowest target index) -- fp64 MFMA distance tiles in the K=4
 * augmented form with a fused running argmin, multiplied only where the tile's bounding box can hold a nearer
 * point (Morton-sorted operands).  idx i32 [n], d2 f64 [n] (direct squared distance of the chosen pair). */
size_t kpx_nn_workspace_bytes(int64_t n_src, int64_t n_tgt);
int kpx_nn_search(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const double *d_T,
                  int32_t *idx, double *d2, void *ws, size_t ws_bytes, void *stream);

/* [O3D] evaluate_registration + get_information_matrix_from_point_clouds at one transformation, without an ICP: the
 * correspondence search of kpx_nn_search (the engine kpx_nn_engine selects), then one deterministic fp64 reduction over the
 * rows with d2 < max_dist^2 (the test of the ICP accumulation, strict).  d_T device f64 [16].
 * d_result device f64 [40]: fitness = count / n_src, inlier_rmse = sqrt(sum d2 / count) (0 when count is 0), count, sum d2,
 * then the 6x6 information matrix row-major: sum G^T G with G = [-[t]x | I3] of the matched TARGET points t (rotation block
 * first, Open3D's order).  The block is bit-identical across the three engines and from run to run.
 * idx i32 [n_src] / d2 f64 [n_src]: the correspondences as kpx_nn_search gives them; either may be NULL. */
size_t kpx_registration_eval_workspace_bytes(int64_t n_src, int64_t n_tgt);
int kpx_registration_eval(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const double *d_T,
                          double max_dist, double *d_result, int32_t *idx, double *d2, void *ws, size_t ws_bytes,
                          void *stream);

/* TransformationEstimationPointToPoint().compute_transformation(src, tgt, corr)
 * (manual_pointcloud_registration.py:90-91): Umeyama/Kabsch without scale on explicit pairs.
 * corr i32 [n_corr*2] = (source index, target index); d_T f64 [16]. */
size_t kpx_kabsch_workspace_bytes(int64_t n_corr);
int kpx_kabsch(const float *src, const float *tgt, const int32_t *corr, int64_t n_corr, double *d_T, void *ws,
               size_t ws_bytes, void *stream);

/* registration_icp(source, target, max_dist, init, estimation, criteria) -- the whole loop runs on
 * the device without host synchronisation.  mode 0 = point-to-point (Kabsch, a16), 1 = point-to-plane
 * (needs tgt_normals, a14).  h_init: f64 [16] host.  d_result f64 [20]: T (16), fitness, inlier_rmse,
 * iterations done, correspondence count.  idx/d2 (optional) receive the last correspondence set: the
 * nearest target of every source point, or idx = -1 / d2 = +inf where no target lies within max_dist
 * (such points are not correspondences).
 * poll_interval == 0: every iteration is enqueued up front and later launches return at once after
 * convergence (fully asynchronous).  poll_interval = p > 0: the host reads the device `done` flag every
 * p iterations (one 4-byte copy + stream sync) and stops enqueuing. */
#define KPX_ICP_POINT_TO_POINT 0
#define KPX_ICP_POINT_TO_PLANE 1
/* kpx_frame_params.icp_mode only (round 5): no registration inside the frame -- the reference registers on its first frame only
 * (preprocessing/data.py:35-41: `if i == 0: ...register...`, every later frame reuses registration_transformations): h_init ARE the
 * transforms, the frame is extract (mask + gate + colour) -> transform + vstack + voxel -> remove_statistical_outlier.  Not taken by
 * kpx_frame_step_sharded. */
#define KPX_ICP_FIXED 2
size_t kpx_icp_workspace_bytes(int64_t n_src, int64_t n_tgt);
int kpx_icp(const float *src, int64_t n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
            double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness,
            double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
            size_t ws_bytes, void *stream);

/* ---- global registration (rows a11-a13) ------------------------------------------------- */

/* compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) (preprocessing/registration.py:15-20).
 * fpfh: f64 [n][33] (Open3D's Feature.data is the transpose, (33, n)).  Needs normals.  max_nn <= KPX_NORMALS_MAX_NN. */
size_t kpx_fpfh_workspace_bytes(int64_t n, int32_t max_nn);
int kpx_fpfh(const float *pts, const float *normals, int64_t n, double radius, int32_t max_nn, double *fpfh, void *ws,
             size_t ws_bytes, void *stream);

/* 1-nearest neighbour of every row of fa among the rows of fb in the 33-D feature space (the matching stage of
 * registration_ransac_based_on_feature_matching, registration.py:50-57); ties to the lowest index. */
size_t kpx_feature_nn_workspace_bytes(int64_t na, int64_t nb);
int kpx_feature_nn(const double *fa, int64_t na, const double *fb, int64_t nb, int32_t *idx, void *ws, size_t ws_bytes,
                   void *stream);

/* RegistrationRANSACBasedOnCorrespondence: ransac_n = 3 correspondences per hypothesis (Philox-seeded, with
 * replacement), Umeyama without scale, CorrespondenceCheckerBasedOnEdgeLength(edge_similarity) and
 * ...BasedOnDistance(max_dist), validation by the full nearest-neighbour correspondence count within max_dist,
 * RANSACConvergenceCriteria(max_iteration, confidence).  Synchronous (the exit test needs each batch's result).
 * corres: i32 [n_corres][2] (source, target) on the device.
 * h_result (host) f64 [20]: T (16) | fitness | inlier_rmse | iterations run | validations. */
size_t kpx_ransac_workspace_bytes(int64_t n_src, int64_t n_tgt);
int kpx_ransac_corres(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                      double max_dist, int32_t ransac_n, double edge_similarity, int32_t max_iteration, double confidence,
                      uint64_t seed, double *h_result, void *ws, size_t ws_bytes, void *stream);

/* Fast Global Registration (Zhou, Park, Koltun 2016; Open3D's FastGlobalRegistration.cpp; tests/fgr_ref.py is the pinned
 * statement).  corres: i32 [n_corres][2] (source, target) on the device; an index outside its cloud is KPX_ERR_RANGE, raised
 * before any point is read and before any output is written.  Both calls are synchronous.
 * kpx_fgr_tuple_test: 100 n_corres trials; trial t draws three correspondences with replacement (Philox counter (0, t, 2, 0),
 *     key = seed) and passes when l_k tuple_scale < m_k < l_k / tuple_scale for the three edge lengths l (source) and m (target).
 *     d_pairs: i32 [3 min(maximum_tuple_count, 100 n_corres)][2], the three pairs of each of the first maximum_tuple_count
 *     passing trials in trial order; d_count: the number of pairs written (device).
 * kpx_fgr_optimize: both clouds normalised by their means and the largest radius (use_absolute_scale: by the means only),
 *     iteration_number Gauss-Newton rounds under the weight (par / (|r|^2 + par))^2 in one launch, par divided by
 *     division_factor after every fourth round while it exceeds maximum_correspondence_distance (decrease_mu).
 *     h_result (host) f64 [20]: T source -> target in the clouds' units (16) | final par | rounds run | failed solves |
 *     largest radius.  n_corres == 0 or iteration_number == 0: the identity. */
size_t kpx_fgr_workspace_bytes(int64_t n_corres);
int kpx_fgr_tuple_test(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                       double tuple_scale, int32_t maximum_tuple_count, uint64_t seed, int32_t *d_pairs, int32_t *d_count,
                       void *ws, size_t ws_bytes, void *stream);
int kpx_fgr_optimize(const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const int32_t *corres, int64_t n_corres,
                     double division_factor, int32_t use_absolute_scale, int32_t decrease_mu, double maximum_correspondence_distance,
                     int32_t iteration_number, double *h_result, void *ws, size_t ws_bytes, void *stream);

/* Several registrations onto ONE shared target (preprocessing/data.py:144-161 registers every sub device onto
 * the master cloud).  The target operand is prepared once; the problems' iterations are queued round-robin on
 * `stream` and each problem's convergence flag is polled through a side stream that waits only for that
 * problem, so the host round trip is hidden behind the other problems' sweeps (kernels never overlap).
 * h_src / h_n_src: host arrays of `count` entries; h_init: count x 16; d_results: count x 20 (as kpx_icp).
 * 1 <= count <= 64: kpx_icp_batch refuses any other batch, and the size query answers 0 for it. */
size_t kpx_icp_batch_workspace_bytes(int32_t count, const int64_t *h_n_src, int64_t n_tgt);
int kpx_icp_batch(int32_t count, const float *const *h_src, const int64_t *h_n_src, const float *tgt,
                  const float *tgt_normals, int64_t n_tgt, double max_dist, const double *h_init, int32_t mode,
                  int32_t max_iteration, double relative_fitness, double relative_rmse, double *d_results, void *ws,
                  size_t ws_bytes, void *stream);

/* The correspondence searches above have two interchangeable implementations with identical results: the culled
 * sweep (default) and the all-pairs sweeps it replaced (fp64 MFMA + float32 screening), kept as an independent
 * cross-check and for A/B measurements.  kpx_nn_engine(e) selects one for the following calls and returns the
 * engine that was active (e < 0: query only).  Initial value: environment KPX_NN_ENGINE=dense|culled. */
#define KPX_NN_ENGINE_CULLED 0
#define KPX_NN_ENGINE_DENSE 1
#define KPX_NN_ENGINE_DENSE_FP64 2 /* the all-pairs engine with every search on the fp64 MFMA sweep (no float32 screening) */
int kpx_nn_engine(int32_t engine);

/* ---- the sampler / normaliser after the path ------------------------------------ */
/* select_points_randomly (utils/processing.py:259-275): number_of_points of the cloud without replacement.  The
 * reference draws np.random.choice from NumPy's unseeded global generator; here point i gets the 64-bit key
 * Philox4x32-10(ctr = (i_lo, i_hi, 'SAMP', 0), key = seed) words (1:0) and the sample is the k points with the
 * smallest (key, i), in that order -- a uniformly random ordered k-subset.  k > n is an error (NumPy raises
 * ValueError).  out_pts (k,3) f32 and/or out_idx (k) i32 on the device; either may be NULL. */
size_t kpx_sample_workspace_bytes(int64_t n);
int kpx_sample_points(const float *pts, int64_t n, int64_t k, uint64_t seed, float *out_pts, int32_t *out_idx, void *ws,
                      size_t ws_bytes, void *stream);

/* PointCloud.get_oriented_bounding_box() for `count` clouds of n points each, stored back to back (the batch arrays of
 * utils/normalization.py:38-42, 74-77, 105-106; one cloud: utils/processing.py:341-344).  Open3D's CreateFromPoints:
 * convex hull, PCA of the hull vertices (eigenvectors by descending eigenvalue, third = first x second; here each of
 * the first two has its largest component positive), box of R^T (v - mean).  pts: f32 (pts_f64 = 0) or f64 (1)
 * [count][n][3] on the device.  d_obb f64 [count][16]: R row-major (9) | centre (3) | extent (3) | number of hull
 * vertices, or -1 (fewer than 3 distinct points / all on one line), -2 (hull did not close), -3 (flat hull: Qhull
 * raises for these).  d_is_vertex: optional u8 [count][n] hull-vertex flags.  Asynchronous. */
size_t kpx_obb_workspace_bytes(int32_t count, int64_t n);
int kpx_obb_batch(const void *pts, int32_t pts_f64, int32_t count, int64_t n, double *d_obb, uint8_t *d_is_vertex, void *ws,
                  size_t ws_bytes, void *stream);

/* The normalisations, applied to `count` groups of `rows` f64 triples (points or joints) with the boxes of kpx_obb_batch:
 *   KPX_NORM_OBB            (x @ M + centre) / max(extent), M = get_rotation_matrix_from_yxz([0, pi, 0])
 *                           (obb_normalization_batch, utils/normalization.py:16-64, as written there)
 *   KPX_NORM_OBB_ROT_TRANS  (x - centre) @ R @ M, M = Rz(90 deg)   (obb_rotation_translation_batch, :67-97)
 *   KPX_NORM_TRANSLATE      x - centre                              (translation_normalization_batch, :100-126)
 *   KPX_NORM_OBB_ROT        (x - centre) @ R                        (obb_normalization, utils/processing.py:329-354)
 * h_M: host 3x3 row-major constant matrix of the mode (NULL where unused). */
#define KPX_NORM_OBB 0
#define KPX_NORM_OBB_ROT_TRANS 1
#define KPX_NORM_TRANSLATE 2
#define KPX_NORM_OBB_ROT 3
int kpx_normalize_batch(const double *x, int32_t count, int64_t rows, const double *d_obb, int32_t mode, const double *h_M,
                        double *out, void *stream);

/* a15: coloured ICP (execute_colored_ICP_registration, preprocessing/registration.py:89-114), SURVEY 8f rank 4.
 * kpx_color_gradient = [O3D] InitializePointCloudForColoredICP: per target point the least-squares gradient of the
 * intensity (r + g + b) / 3 in its tangent plane over the hybrid neighbourhood (radius, max_nn; Open3D passes
 * 2 x max_correspondence_distance and 30); grad f64 [n][3] on the device.
 * kpx_colored_icp = [O3D] registration_colored_icp: the registration_icp loop (correspondences, fitness, inlier rmse,
 * convergence as kpx_icp) with TransformationEstimationForColoredICP(lambda_geometric, Open3D default 0.968) as the
 * update: per pair a geometric row sqrt(lambda) ((s - t).n) and a photometric row sqrt(1 - lambda) (I_s - I_t - g.(s' - t)).
 * colours f32 [n][3]; d_result as kpx_icp. */
size_t kpx_color_gradient_workspace_bytes(int64_t n, int32_t max_nn);
int kpx_color_gradient(const float *pts, const float *normals, const float *colors, int64_t n, double radius, int32_t max_nn,
                       double *grad, void *ws, size_t ws_bytes, void *stream);
size_t kpx_colored_icp_workspace_bytes(int64_t n_src, int64_t n_tgt);
int kpx_colored_icp(const float *src, const float *src_colors, int64_t n_src, const float *tgt, const float *tgt_colors,
                    const float *tgt_normals, const double *tgt_gradient, int64_t n_tgt, double max_dist, const double *h_init,
                    double lambda_geometric, int32_t max_iteration, double relative_fitness, double relative_rmse,
                    int32_t poll_interval, double *d_result, void *ws, size_t ws_bytes, void *stream);

/* Generalized ICP ([O3D] registration_generalized_icp with TransformationEstimationForGeneralizedICP, L2 loss).
 * kpx_gicp_covariances = InitializePointCloudForGeneralizedICP from normals: C = R_x diag(epsilon, 1, 1) R_x^T,
 *   R_x = GetRotationFromE1ToX(n) evaluated literally (identity when n.x < -0.99, Open3D's branch).  cov f64 [n][9].
 * kpx_rotate_covariances: out = R C R^T (R = rotation of the row-major host 4x4 h_T), in == out allowed.
 * kpx_generalized_icp: the kpx_icp loop (correspondences, fitness, inlier rmse, convergence; same argument checks and
 *   d_result layout) with the plane-to-plane update: per pair M = Ct + R Cs R^T, W = M^{-1/2}, three rows (s x w_i, w_i | w_i.(s - t)).
 *   Covariances f64 [n][9] in each cloud's own frame.  A pair with a singular M adds nothing, and a singular 6x6 system gives the
 *   identity update (Open3D yields NaN in both cases).  idx / d2 optional as in kpx_icp. */
int kpx_gicp_covariances(const float *normals, int64_t n, double epsilon, double *cov, void *stream);
int kpx_rotate_covariances(const double *cov, int64_t n, const double *h_T, double *out, void *stream);
size_t kpx_generalized_icp_workspace_bytes(int64_t n_src, int64_t n_tgt);
int kpx_generalized_icp(const float *src, const double *src_cov, int64_t n_src, const float *tgt, const double *tgt_cov, int64_t n_tgt,
                        double max_dist, const double *h_init, int32_t max_iteration, double relative_fitness, double relative_rmse,
                        int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws, size_t ws_bytes, void *stream);

/* Robust registrations: [O3D] TransformationEstimationPointToPlane / ...ForColoredICP / ...ForGeneralizedICP with a RobustKernel.
 * Every residual row r of the update (one per pair for point-to-plane; the two scaled rows sqrt(lambda) r_G and sqrt(1 - lambda) r_I
 * of coloured ICP; the three rows of a GICP pair) enters the normal equations as J^T w J and J^T w r with Open3D's weights
 *   KPX_LOSS_L2      w = 1                         KPX_LOSS_CAUCHY  w = 1 / (1 + (r / k)^2)
 *   KPX_LOSS_L1      w = 1 / |r|                   KPX_LOSS_GM      w = k / (k + r^2)^2
 *   KPX_LOSS_HUBER   w = k / max(|r|, k)           KPX_LOSS_TUKEY   w = (1 - min(1, |r| / k)^2)^2
 * Correspondences, fitness, inlier rmse, the convergence test and so the iteration count do not depend on the loss (as in Open3D).
 * Each entry point takes its L2 sibling's arguments (same checks, same d_result, workspace of kpx_icp_workspace_bytes) plus
 * loss and loss_k, and runs search -> weighted sums -> solve as three launches per iteration on whichever engine kpx_nn_engine
 * selected.  The robust point-to-plane entry accepts KPX_ICP_POINT_TO_PLANE only: Open3D's point-to-point estimation has no kernel.
 * Deviations from Open3D: a row whose weight is not finite adds nothing (Open3D: NaN from L1 at r == 0); loss_k > 0 is required for
 * Huber, Cauchy, GM and Tukey (Open3D does not check k), and ignored for L2 and L1. */
#define KPX_LOSS_L2 0
#define KPX_LOSS_L1 1
#define KPX_LOSS_HUBER 2
#define KPX_LOSS_CAUCHY 3
#define KPX_LOSS_GM 4
#define KPX_LOSS_TUKEY 5
int kpx_icp_robust(const float *src, int64_t n_src, const float *tgt, const float *tgt_normals, int64_t n_tgt,
                   double max_dist, const double *h_init, int32_t mode, int32_t max_iteration, double relative_fitness,
                   double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
                   size_t ws_bytes, void *stream, int32_t loss, double loss_k);
int kpx_colored_icp_robust(const float *src, const float *src_colors, int64_t n_src, const float *tgt, const float *tgt_colors,
                           const float *tgt_normals, const double *tgt_gradient, int64_t n_tgt, double max_dist, const double *h_init,
                           double lambda_geometric, int32_t max_iteration, double relative_fitness, double relative_rmse,
                           int32_t poll_interval, double *d_result, void *ws, size_t ws_bytes, void *stream, int32_t loss,
                           double loss_k);
int kpx_generalized_icp_robust(const float *src, const double *src_cov, int64_t n_src, const float *tgt, const double *tgt_cov,
                               int64_t n_tgt, double max_dist, const double *h_init, int32_t max_iteration, double relative_fitness,
                               double relative_rmse, int32_t poll_interval, double *d_result, int32_t *idx, double *d2, void *ws,
                               size_t ws_bytes, void *stream, int32_t loss, double loss_k);

/* fuse_skeletons_gradient (utils/skeleton_fusion.py:21-74), SURVEY 8f rank 4: gradient- and centroid-weighted average of the
 * joints seen by three cameras.  skeletons f64 [cams][frames][joints][3] on the device; the first initial_frame (reference: 20)
 * frames are the mean over ALL cameras, later frames weight the FIRST THREE cameras (as the reference does) with
 * w_c = 1 / (|p_c - fused[f-1]|^alpha |p_c - centroid|^beta).  out f64 [frames][joints][3]. */
int kpx_fuse_skeletons(const double *skeletons, int32_t cams, int64_t frames, int32_t joints, double alpha, double beta,
                       int32_t initial_frame, double *out, void *stream);

/* ---- the frame loop as one native call ------------------------------------------------------------------------------- */
/* One synchronised frame set of `sensors` devices held by this GPU: the body of DataProcessor's frame loop
 * (preprocessing/data.py:35-61) with the registration of data.py:127-161 on the same depth images folded in --
 *   depth -> full cloud -> voxel_down_sample(reg_voxel) per sensor; normals of the master's (sensor 0);
 *   execute_point_to_plane_registration of every sub sensor onto the master (h_init: the sensors - 1 initial 4x4, host);
 *   depth + person mask (rgb with the background zeroed, data.py:169) + depth gate -> the person clouds;
 *   pcd.transform(T_i) + np.vstack + voxel_down_sample(filt_voxel) in one fp64 pass; remove_statistical_outlier(filt_k, filt_ratio).
 * Host orchestration in C++ over the entry points above (the Python mirror of this loop is kinectpy_amd/pipeline.py): one
 * call per frame, synchronous (the data-dependent counts are read back on `stream` inside); when it returns the selection
 * kernel that writes out_pts / out_col is queued on `stream`.  depth u16 [sensors][n_px], rgb u8 [sensors][n_px][3], xy_table
 * f32 [n_px][2] on the device; out_pts / out_col f32 [sensors * n_px][3] worst case; h_count: points written; h_T f64
 * [sensors][16] (identity for the master); h_info (optional, 64 ints): [0..15] down-sampled points per sensor, [16..31] masked
 * points per sensor, [32..47] ICP iterations per sensor, [48] voxels of the fused cloud. */
typedef struct {
    double reg_voxel;          /* 35   preprocessing/registration.py:35,69 */
    double icp_max_dist;       /* 100  registration.py:75 */
    double filt_voxel;         /* filter_outliers voxel_size (filtering.py:16) */
    double filt_ratio;         /* filter_outliers std_ratio */
    double gate;               /* 750  data.py:170-171 */
    int32_t normals_nn;        /* 40   registration.py:24 */
    int32_t icp_mode;          /* KPX_ICP_POINT_TO_PLANE (registration.py:83) */
    int32_t icp_max_iteration; /* 30   Open3D's default criteria */
    int32_t filt_k;            /* filter_outliers nb_neighbors */
} kpx_frame_params;
size_t kpx_frame_step_workspace_bytes(int32_t sensors, int64_t n_px);
int kpx_frame_step(const uint16_t *depth, const uint8_t *rgb, const float *xy_table, int64_t n_px, int32_t sensors,
                   const double *h_init, const kpx_frame_params *params, float *out_pts, float *out_col, int32_t *h_count,
                   double *h_T, int32_t *h_info, void *ws, size_t ws_bytes, void *stream);
/* The same frame handed over in HOST memory (pinned for an asynchronous copy) -- SURVEY 8(d)'s interval "depth frame resident in
 * host pinned memory -> fused registered cloud on the GPU"; the reference's loop starts from the files it has just read
 * (preprocessing/data.py:87-124).  h_depth u16 [sensors][n_px], h_rgb u8 [sensors][n_px][3] on the host; both are copied into
 * staging buffers at the head of `ws` on `stream` (no allocation, no extra synchronisation), then kpx_frame_step runs. */
size_t kpx_frame_step_host_workspace_bytes(int32_t sensors, int64_t n_px);
int kpx_frame_step_host(const uint16_t *h_depth, const uint8_t *h_rgb, const float *xy_table, int64_t n_px, int32_t sensors,
                        const double *h_init, const kpx_frame_params *params, float *out_pts, float *out_col, int32_t *h_count,
                        double *h_T, int32_t *h_info, void *ws, size_t ws_bytes, void *stream);

/* ---- the frame loop over several GPUs (preprocessing/data.py:96-122 loops the devices independently, :44-61 fuses and
 * filters, :127-161 registers every sub device onto the master) -------------------------------------------------------------------
 * One PROCESS per GPU, sensor g on GPU g (fewer GPUs than sensors: contiguous blocks in rank order).  The host side of a frame runs
 * in C++; its three collectives -- master cloud broadcast, all-gather of the masked clouds + registration results, all-gather of
 * the fused filter's slab distances -- are issued from here on the frame's stream.
 *
 * kpx_comm: one communicator over all ranks (one per frame slot when several frames are in flight).  Transports:
 *   RCCL        kpx_rccl_load(path of librccl.so, NULL = the loader's search path) once per process; rank 0 draws a 128-byte id
 *               (kpx_rccl_unique_id) and hands it to the other ranks by any means (e.g. torch.distributed.broadcast_object_list);
 *               every rank then calls kpx_comm_create_rccl (collective, like ncclCommInitRank);
 *   callbacks   kpx_comm_create_callbacks: the caller moves the bytes (host-staged gloo, in-process ranks): rehearsals without RCCL.
 * The callbacks get device pointers and the frame's stream; they return 0 on success. */
typedef struct kpx_comm kpx_comm;
typedef int (*kpx_bcast_fn)(void *user, void *d_buf, size_t bytes, int32_t root, void *stream);
typedef int (*kpx_allgather_fn)(void *user, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
int kpx_rccl_load(const char *path);
int kpx_rccl_unique_id(void *id128);
int kpx_comm_create_rccl(const void *id128, int32_t rank, int32_t world, kpx_comm **out);
int kpx_comm_create_callbacks(int32_t rank, int32_t world, kpx_bcast_fn bcast, kpx_allgather_fn allgather, void *user, kpx_comm **out);
/* Replay transport (measurement aid of bench.py --emulate-world): ONE rank of a `world`-rank job on one GPU, the peers' messages taken
 * from recordings of a real world-rank run.  d_payloads / bytes: [frames][3][world] device pointers / sizes of what rank r sent in
 * collective c (0 master broadcast -- root's entry only --, 1 cloud exchange, 2 slab all-gather) of recorded frame f.  Call n of the
 * communicator is collective n % 3 of frame (first_frame + stride * (n / 3)) % frames.  Message sizes must be the recording's (both
 * runs with KPX_SHARD_FIXED_CAP=1).  Replaces nothing of the reference: it prices a rank's share of preprocessing/data.py:35-61. */
int kpx_comm_create_replay(int32_t rank, int32_t world, int32_t frames, int32_t first_frame, int32_t stride, int32_t per_frame,
                           const void *const *d_payloads, const size_t *bytes, kpx_comm **out);      /* per_frame: 3, or 2 for frames without collective 2 */
int kpx_comm_destroy(kpx_comm *comm);
int kpx_comm_rank(const kpx_comm *comm);
int kpx_comm_world(const kpx_comm *comm);
/* in-place broadcast of device memory from `root` / all-gather into d_recv [world][bytes_per_rank], on `stream` */
int kpx_comm_broadcast(kpx_comm *comm, void *d_buf, size_t bytes, int32_t root, void *stream);
int kpx_comm_allgather(kpx_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
/* utility for callback transports: copy between any two of host / device memory on `stream`; wait != 0 also waits for the stream */
int kpx_copy_bytes(void *dst, const void *src, size_t bytes, void *stream, int32_t wait);

/* kpx_order: ONE issue order for the collectives of the frames in flight on a rank.  Frames in flight run on host threads; a
 * collective kernel spins on the device until its peers arrive, so every rank must enqueue the collectives of its frames in the
 * same order whatever the timing of its threads: stage s (0 broadcast, 1 exchange, 2 slab all-gather) of frame f has the key 3 f
 * (s = 0) or 3 (f + depth - 1) + s, and a collective is issued only when every smaller key of the submitted frames is done.  The
 * main thread calls submit (a frame enters; -> its number), block(frame) while it waits for that frame (block(-1) afterwards) and
 * finish(frame) when the frame is over; kpx_frame_step_sharded takes its turns itself (turn_begin / turn_end / skip, exported for
 * tests).  A NULL order means one frame at a time. */
typedef struct kpx_order kpx_order;
int kpx_order_create(int32_t depth, kpx_order **out);
int kpx_order_destroy(kpx_order *order);
int kpx_order_submit(kpx_order *order, int64_t *frame);
int kpx_order_block(kpx_order *order, int64_t frame);
int kpx_order_turn_begin(kpx_order *order, int64_t frame, int32_t stage);
int kpx_order_turn_end(kpx_order *order, int64_t frame, int32_t stage);
int kpx_order_skip(kpx_order *order, int64_t frame, int32_t stage);
int kpx_order_finish(kpx_order *order, int64_t frame);
int kpx_order_log(kpx_order *order, int64_t *out, int64_t cap, int64_t *count);

/* kpx_frame_step for the rank's share of the rig.  depth / rgb: the images of THIS rank's sensors (sensor order), on the device or
 * (host_input != 0) in host memory; h_init: the sensors - 1 initial transforms of ALL sub sensors; fused_filter 0 = the filter on
 * the fused cloud is sharded over the ranks by slabs of its grid order (every rank ends with the filtered frame, bit-identical to
 * the one-GPU filter), 1 = rank 0 filters alone (the others return *h_count = 0), 2 = frame f's fused pass and filter run on rank
 * f mod world alone (f: the kpx_order's frame number; the owner returns the frame, the others 0 rows).  h_T f64 [sensors][16] and h_info describe the
 * WHOLE rig on every rank (they travel in the exchange headers).  Message capacities adapt to the slot's previous frame; when a
 * frame outgrows one, every rank returns KPX_RETRY (1) and the caller runs the frame again (a new frame number under a kpx_order).
 * Workspace: kpx_frame_step_sharded_workspace_bytes(sensors, rank, world, n_px, host_input). */
size_t kpx_frame_step_sharded_workspace_bytes(int32_t sensors, int32_t rank, int32_t world, int64_t n_px, int32_t host_input);
int kpx_frame_step_sharded(kpx_comm *comm, kpx_order *order, int64_t frame, const uint16_t *depth, const uint8_t *rgb, int32_t host_input,
                           const float *xy_table, int64_t n_px, int32_t sensors, const double *h_init, const kpx_frame_params *params,
                           int32_t fused_filter, float *out_pts, float *out_col, int32_t *h_count, double *h_T, int32_t *h_info, void *ws,
                           size_t ws_bytes, void *stream);

/* ---- frames in flight, scheduled natively (round 5) -------------------------------------------------
 * The reference's frame loop is sequential (preprocessing/data.py:35-61); consecutive frames are independent, and one frame is a
 * chain of ~100 short dispatches with four read-backs, so `depth` frames run side by side: kpx_stream owns `depth` worker threads
 * (C++, inside the library: no interpreter between a frame's end and the next one's start), each with its own HIP stream and its
 * own slice of the caller's workspace (kpx_stream_workspace_bytes).  kpx_stream_submit hands a frame over and returns at once
 * (KPX_ERR_INVALID when kpx_stream_capacity frames are queued); kpx_stream_pop blocks until the OLDEST frame in flight is done and returns
 * its status, its point count (out_pts / out_col given at submit: rows [0, *h_count) are valid when pop returns, on any stream),
 * transforms (f64 [sensors][16]) and info words (int32 [64], as kpx_frame_step).  depth / rgb of a frame: device memory, or pinned
 * host memory with host_input != 0 (the copy then runs on the slot's stream, inside the frame); they must stay valid until the
 * frame has been popped.  submit / pop / destroy: one calling thread.
 * comms == NULL: one GPU (kpx_frame_step / kpx_frame_step_host per frame).  comms = `depth` communicators, one per slot: the
 * rank's share of the rig through kpx_frame_step_sharded, the collectives of the frames in flight in ONE issue order on every rank
 * (a kpx_order owned by the stream); a frame that outgrew its messages on every rank alike is run again inside kpx_stream_pop. */
typedef struct kpx_stream kpx_stream;
size_t kpx_stream_workspace_bytes(int32_t sensors, int32_t rank, int32_t world, int64_t n_px, int32_t depth);
int kpx_stream_create(const float *xy_table, int64_t n_px, int32_t sensors, const double *h_init, const kpx_frame_params *params,
                      int32_t depth, kpx_comm *const *comms, int32_t fused_filter, void *ws, size_t ws_bytes, kpx_stream **out);
int kpx_stream_submit(kpx_stream *stream, const void *depth, const void *rgb, int32_t host_input, float *out_pts, float *out_col);
int kpx_stream_pop(kpx_stream *stream, int32_t *h_count, double *h_T, int32_t *h_info);
int kpx_stream_pending(const kpx_stream *stream);
int kpx_stream_capacity(const kpx_stream *stream);    /* frames kpx_stream_submit takes before a pop: 2 x depth on one GPU (one queue, any free worker
                                                         takes the oldest frame), depth with communicators (frame j runs on slot j % depth on every rank) */
int kpx_stream_destroy(kpx_stream *stream);
/* h_out4: [0] frames finished by the stream's workers, [1..3] reserved: always 0 (they reported an all-frames ICP scheduler that
 * was measured slower than a chain of launches per frame and removed: DESIGN.md section 5.2). */
int kpx_stream_stats(const kpx_stream *stream, uint64_t *h_out4);

/* What the library's per-thread owners hold right now, summed over the host threads of the process:
   h_out4[0] bytes of pinned host memory, [1] internal HIP streams, [2] HIP events, [3] threads holding any.
   Host arithmetic only; all zero in a process that never touched a GPU. */
int kpx_host_resources(uint64_t *h_out4);

/* ---- measurement hooks (bench.py) --------------------------------------------------------------- */
/* HIP-event timing of the hot kernels on the stream they are launched on.  kpx_prof_begin arms it
 * (capacity = max launches recorded); every launch of a tagged kernel is bracketed by an event pair;
 * kpx_prof_end synchronises, sums per kernel id and disarms.  h_ms / h_launches / h_work: arrays of
 * KPX_PROF_KERNELS entries (work = flops for the MFMA kernels -- for NN_LOCAL the flops of the tiles actually
 * multiplied, counted on the device -- and algorithmic bytes for the others). */
#define KPX_PROF_NN_MFMA 0
#define KPX_PROF_SOR_KNN 1
#define KPX_PROF_PLANE_SCORE 2
#define KPX_PROF_COMPACT 3
#define KPX_PROF_NN_SCREEN 4
#define KPX_PROF_NN_LOCAL 5
#define KPX_PROF_KERNELS 6
int kpx_prof_begin(int32_t capacity);
/* Time only every stride-th launch of each kernel id (default 1).  An event pair costs ~2 us of stream time; around
 * every launch of a 16 us kernel that is measurable in the end-to-end number (bench.py uses 8). */
int kpx_prof_stride(int32_t stride);
int kpx_prof_end(double *h_ms, int64_t *h_launches, double *h_work);
/* Device-side phase clock of the ICP iteration kernel (stamps while the profiler is armed), LAST launch: h_out8 = average
 * microseconds a block spends in [0] the update prologue, [1] row preparation, [2] the culled sweep, [3] the pair epilogue,
 * [4] the block sums; [5] blocks; [6] latest - earliest block start (dispatch ramp); [7] earliest start -> latest end;
 * [8..12] the slowest block of each phase; [13] the longest block lifetime; [14] blocks the launch did not sweep because they
 * provably had no partner within reach.  h_out8 holds 16 doubles. */
int kpx_prof_icp_phases(double *h_out8);
/* Per-wave rows of the same launch (4 x uint64 per wave: sweep start, sweep end in 10 ns ticks; counters = tiles multiplied |
 * tile-box fetches << 16 | operand fetches << 32 | groups kept << 48; sampled rows with a partner).  *h_count = the number of
 * waves written (<= cap_waves). */
int kpx_prof_icp_waves(uint64_t *h_out, int64_t cap_waves, int64_t *h_count);
/* The one-launch form of the culled ICP chain (kpx_icp_batch groups whose blocks fit the device; kpx_icp.hip, icp_chain_kernel): on = 1 / 0
   switches it for the calling process, on = -1 only asks; returns the previous setting (on = -2: the number of chains this process has launched).  Default: on unless KPX_ICP_CHAIN=0.  Results do
   not depend on it (tests/test_parity_gpu.py, test_icp_update_placements_and_light_skip_are_bit_identical). */
int kpx_icp_chain(int32_t on);
/* Self-check of the row certificates of the culled ICP sweep (kpx_icp_batch with KPX_ICP_CERT_CHECK=1 in the environment: rows whose
 * partner is certified unchanged -- registration_icp's correspondence step, preprocessing/registration.py:78-84 -- are searched all
 * the same and compared).  h_out8 (8 x uint64, cleared by the call): [0] rows certified, [1] rows searched, [2] certified rows whose
 * search found another partner (must be 0), [3..7] the first such row: iteration, sorted row, kept and found partner, key bits. */
int kpx_prof_icp_cert(uint64_t *h_out8);
/* Clock of the one-launch ICP chain (KPX_ICP_CHAIN_STAMPS=1): 64 iterations x 48 stamps of the 100 MHz wall clock, first registration of
   the last chain launch (slots: kpx_icp.hip, g_chain_stamp); read and reset.  A development aid like the other kpx_prof_* entries. */
int kpx_prof_icp_chain(uint64_t *h_out3072);

/* ---- volumetric integration ([O3D] pipelines.integration.UniformTSDFVolume; arithmetic contract AC9) ------------ */
/* The volume is caller-owned and zero-initialised by the caller (reset = clear it): volume f32 [res^3][2] = {tsdf, weight} per
 * voxel, 16-byte aligned; color f32 [res^3][3] or NULL (no colours); voxel (x, y, z) at linear index (x res + y) res + z; its
 * centre is h_origin + (index + 0.5) voxel_length.  1 <= resolution <= KPX_TSDF_MAX_RESOLUTION.
 * kpx_tsdf_integrate: `count` images of width x height pixels, taken with the pinhole h_intrinsic = (fx, fy, cx, cy) from the
 *     poses h_extrinsics f64 [count][16] (world -> camera, row-major 4x4, host), are integrated in ascending order: every voxel
 *     whose centre projects into image s at a pixel of depth d > 0 with sdf = (d - z) sqrt(xm^2 + ym^2 + 1) > -sdf_trunc takes
 *     tsdf = (tsdf w + min(1, sdf / sdf_trunc)) / (w + 1) (colours alike), w += 1.  The result equals `count` calls with one image
 *     each, bit for bit; one launch holds up to KPX_TSDF_MAX_SENSORS images (one read and one write of a voxel for all of them),
 *     larger counts run as consecutive launches.  h_depth: host array of device pointers, f32 [H W] (depth_u16 = 0; depth_scale
 *     and depth_trunc are ignored) or u16 [H W] (depth_u16 = 1: d = (float)raw / (float)depth_scale, d > (float)depth_trunc -> 0,
 *     what RGBDImage.create_from_color_and_depth computes).  h_rgb: host array of device pointers u8 [H W 3]; read only when
 *     color is given (then required).  Asynchronous.
 * kpx_tsdf_extract_count / kpx_tsdf_extract_fill: the two phases of extract_point_cloud (KPX_TSDF_SURFACE: one point per zero
 *     crossing between a valid voxel -- w != 0, -0.98 <= tsdf < 0.98 -- and its valid +x / +y / +z neighbour, ascending in (linear
 *     index, axis), with normals and, from a colour volume, colours) and of extract_voxel_point_cloud (KPX_TSDF_VOXELS: the centre
 *     of every valid voxel, ascending, colour = grey (tsdf + 1) / 2).  count writes one count per KPX_TSDF_COUNT_BLOCK consecutive
 *     voxels into ws, scans them there and leaves the total at d_count (i64, device).  The caller reads it, allocates pts / nrm /
 *     col f32 [total][3] and calls fill with the SAME, untouched ws and an unchanged volume.  nrm and col may be NULL (not
 *     wanted); col needs `color` in the surface mode.  fill writes nothing at or beyond `total`.  Asynchronous.
 * ws: kpx_tsdf_workspace_bytes(resolution) bytes (0 for a resolution outside the range). */
#define KPX_TSDF_MAX_RESOLUTION 1024
#define KPX_TSDF_MAX_SENSORS 8
#define KPX_TSDF_COUNT_BLOCK 512
#define KPX_TSDF_SURFACE 0
#define KPX_TSDF_VOXELS 1
size_t kpx_tsdf_workspace_bytes(int32_t resolution);
int kpx_tsdf_integrate(float *volume, float *color, int32_t resolution, double voxel_length, const double *h_origin, double sdf_trunc,
                       int32_t count, const void *const *h_depth, int32_t depth_u16, double depth_scale, double depth_trunc,
                       const uint8_t *const *h_rgb, int32_t width, int32_t height, const double *h_intrinsic, const double *h_extrinsics,
                       void *stream);
int kpx_tsdf_extract_count(const float *volume, int32_t resolution, int32_t mode, int64_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_tsdf_extract_fill(const float *volume, const float *color, int32_t resolution, double voxel_length, const double *h_origin,
                          int32_t mode, int64_t total, float *pts, float *nrm, float *col, void *ws, size_t ws_bytes, void *stream);

/* ---- block-sparse integration ([O3D] pipelines.integration.ScalableTSDFVolume; arithmetic contract AC16) ------- */
/* Blocks of R^3 voxels (R = unit_resolution in [1, KPX_TSDF_BLOCKS_MAX_RESOLUTION]) on the world lattice: block (bx, by, bz) spans
 * [b ul, (b + 1) ul) per axis, ul = voxel_length R, voxel (x, y, z) of it at local index (x R + y) R + z, centre b ul + (index + 0.5)
 * voxel_length.  All storage is the caller's: pool f32 [capacity][R^3][2] = {tsdf, weight}, color_pool f32 [capacity][R^3][3] or
 * null, and the index: index_keys i64 [n_blocks] ascending, key = (bx + 2^20) << 42 | (by + 2^20) << 21 | (bz + 2^20), index_slots
 * i32 [n_blocks] the pool slot of each.  Every call is asynchronous on `stream`.
 * kpx_tsdf_blocks_touch: the blocks `count` (1..KPX_TSDF_MAX_SENSORS) images touch: of every stride-th pixel of every stride-th row
 *     with depth > 0 (f32 images, or u16 with depth_scale / depth_trunc as kpx_tsdf_integrate) the world point h_poses[s] (x, y, z, 1)
 *     (camera -> world, f64 row-major 4x4 each; fma chain as in AC1) and every block of the box floor((p -+ sdf_trunc) / ul).
 *     0 < sdf_trunc <= unit_length.  d_counts i64 [3] = {touched blocks, touched blocks that are not in the index, 1 when a block index
 *     left [-2^20, 2^20) -- KPX_ERR_RANGE for the caller to raise -- else 0}.  The workspace keeps the touched keys ascending, their
 *     image masks and pool slots (a new block: n_blocks + its rank among the new ones) for the two calls below, which take the same
 *     count / width / height / stride / unit_length / sdf_trunc.  ws: kpx_tsdf_blocks_touch_workspace_bytes (0 for a bad shape).
 * kpx_tsdf_blocks_insert: out_keys / out_slots [n_blocks + n_new] = the index merged with the touch's n_new new keys (slots n_blocks,
 *     n_blocks + 1, ... in ascending key order); zeroes those pool slots.  capacity >= n_blocks + n_new.
 * kpx_tsdf_blocks_integrate: AC9's update of every voxel of the touch's n_touched blocks by the images of each block's mask, ascending;
 *     h_extrinsics world -> camera as kpx_tsdf_integrate.  A block is read and written at most once.
 * kpx_tsdf_blocks_extract_count / _fill, kpx_tsdf_blocks_mesh_count / _fill: as the uniform volume's four, over the voxels of the
 *     existing blocks in ascending (key, local index); neighbours, interpolation taps and cube corners are taken by global voxel index
 *     and may lie in adjacent blocks; an absent block gives no crossing, taps of 0 and inactive cubes.  There is no origin and no last-
 *     layer exclusion.  ws: kpx_tsdf_blocks_extract_workspace_bytes(n_blocks, R, mesh), carried from count to fill. */
#define KPX_TSDF_BLOCKS_MAX_RESOLUTION 32
size_t kpx_tsdf_blocks_touch_workspace_bytes(int32_t count, int32_t width, int32_t height, int32_t stride, double unit_length, double sdf_trunc);
int kpx_tsdf_blocks_touch(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, int32_t count, const void *const *h_depth,
                          int32_t depth_u16, double depth_scale, double depth_trunc, int32_t width, int32_t height, const double *h_intrinsic,
                          const double *h_poses, int32_t stride, double unit_length, double sdf_trunc, int64_t *d_counts, void *ws,
                          size_t ws_bytes, void *stream);
int kpx_tsdf_blocks_insert(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, int64_t n_new, int64_t *out_keys,
                           int32_t *out_slots, float *pool, float *color_pool, int64_t capacity, int32_t unit_resolution, int32_t count,
                           int32_t width, int32_t height, int32_t stride, double unit_length, double sdf_trunc, const void *ws, size_t ws_bytes,
                           void *stream);
int kpx_tsdf_blocks_integrate(float *pool, float *color_pool, int64_t capacity, int32_t unit_resolution, double voxel_length, double sdf_trunc,
                              int64_t n_touched, int32_t count, const void *const *h_depth, int32_t depth_u16, double depth_scale,
                              double depth_trunc, const uint8_t *const *h_rgb, int32_t width, int32_t height, const double *h_intrinsic,
                              const double *h_extrinsics, int32_t stride, const void *ws, size_t ws_bytes, void *stream);
size_t kpx_tsdf_blocks_extract_workspace_bytes(int64_t n_blocks, int32_t unit_resolution, int32_t mesh);
int kpx_tsdf_blocks_extract_count(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                                  int32_t unit_resolution, int32_t mode, int64_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_tsdf_blocks_extract_fill(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                                 const float *color_pool, int32_t unit_resolution, double voxel_length, int32_t mode, int64_t total, float *pts,
                                 float *nrm, float *col, void *ws, size_t ws_bytes, void *stream);
int kpx_tsdf_blocks_mesh_count(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                               int32_t unit_resolution, int64_t *d_counts, void *ws, size_t ws_bytes, void *stream);
int kpx_tsdf_blocks_mesh_fill(const int64_t *index_keys, const int32_t *index_slots, int64_t n_blocks, const float *pool,
                              const float *color_pool, int32_t unit_resolution, double voxel_length, int64_t n_vertices, int64_t n_triangles,
                              float *out_vertices, float *out_colors, int32_t *out_triangles, void *ws, size_t ws_bytes, void *stream);

/* ---- triangle meshes ([O3D] UniformTSDFVolume.extract_triangle_mesh, geometry.TriangleMesh; arithmetic contract AC12, DESIGN.md 3 /
 *      5.11) ------------------------------------------------------------------------------------------------------------------------ */
/* kpx_tsdf_mesh_count / kpx_tsdf_mesh_fill: the two phases of marching cubes over a volume laid out as above.  A cube (x, y, z), every
 *     index below res - 1, is active when its eight corner weights are != 0; bit i of its code is tsdf_i < 0 (corner and edge numbering:
 *     kinectpy_amd/csrc/kpx_mctables.h); codes 0 and 255 emit nothing; there is no +-0.98 test.  One vertex per edge (lower voxel v, axis
 *     a) that some active cube contains and whose ends differ in sign: centre of v, moved along a by (|f_v| vl) / (|f_v| + |f_v+a|), plus
 *     h_origin; colour (|f_v+a| (c_v / 255) + |f_v| (c_v+a / 255)) / (|f_v| + |f_v+a|) per channel; all fp64 without fma, rounded to
 *     f32 at the store.  Vertices ascend in (linear index of v, a) -- Open3D numbers them by first encounter; positions and the triangle
 *     list modulo that renumbering are Open3D's.  Triangles: cubes in ascending linear index, the table row in order, every triple (t0,
 *     t1, t2) emitted as (vertex[t0], vertex[t2], vertex[t1]).  count leaves its records in ws and the two totals at d_counts (i64 [2],
 *     device: vertices, triangles).  The caller reads them, allocates out_vertices f32 [n_vertices][3], out_colors (optional, needs
 *     `color`) and out_triangles i32 [n_triangles][3] and calls fill with the SAME, untouched ws and an unchanged volume; fill writes
 *     nothing at or beyond the two counts and returns KPX_ERR_RANGE when either exceeds 2^31 - 1.  Asynchronous.
 *     ws: kpx_tsdf_mesh_workspace_bytes(resolution) bytes (0 for a resolution outside the range): 1.5 bytes per voxel.
 * kpx_mesh_normals: triangle normal n = (v1 - v0) x (v2 - v0) in fp64 from the f32 vertices, each component a b - c d; vertex normal =
 *     the sum from 0 of the UNNORMALISED normals of the incident triangles in ascending triangle index, once per corner occurrence.
 *     normalized: n / sqrt((nx^2 + ny^2) + nz^2), the zero vector -> (0, 0, 1).  Stored as f32.  Either output may be NULL.  Every
 *     triangle index must lie in [0, n_vertices): the caller checks (a triangle that violates it reads nothing and counts as n = 0).
 *     At most 2^31 - 1 vertices and triangle corners (KPX_ERR_RANGE).  ws: kpx_mesh_normals_workspace_bytes (0 for counts out of range),
 *     needed for vertex normals only.  Asynchronous.
 * kpx_mesh_surface_area: d_area (f64, device) = the sum over the triangles, in ascending order, of sqrt(...) of that n times 0.5.
 *     The additions are one chain by contract (one block; about 3 ns per triangle).  Asynchronous. */
size_t kpx_tsdf_mesh_workspace_bytes(int32_t resolution);
int kpx_tsdf_mesh_count(const float *volume, int32_t resolution, int64_t *d_counts, void *ws, size_t ws_bytes, void *stream);
int kpx_tsdf_mesh_fill(const float *volume, const float *color, int32_t resolution, double voxel_length, const double *h_origin,
                       int64_t n_vertices, int64_t n_triangles, float *out_vertices, float *out_colors, int32_t *out_triangles, void *ws,
                       size_t ws_bytes, void *stream);
size_t kpx_mesh_normals_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_normals(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, int32_t normalized,
                     float *out_triangle_normals, float *out_vertex_normals, void *ws, size_t ws_bytes, void *stream);
int kpx_mesh_surface_area(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double *d_area, void *stream);

/* ---- mesh clean-up ([O3D] geometry.TriangleMesh; arithmetic contract AC13) ------------------------------------------
 * Every operator takes float32 vertices / colours / normals [n][3] and int32 triangles [n_triangles][3] in device memory, works on
 * `stream` and returns without waiting.  Every triangle index must lie in [0, n_vertices): the caller checks; a triangle that violates
 * it reads nothing, makes no pair and no edge, has area 0 and is a cluster of its own.  At most 2^31 - 1 vertices and 6 n_triangles
 * (KPX_ERR_RANGE); the workspace queries return 0 for counts outside that.  All floating-point work is fp64, every multiply and add
 * separate; values round to float32 only where stated.
 * kpx_mesh_adjacency: N(v) = the ascending distinct vertices that share a corner pair of some triangle with v (a triangle (a, a, b)
 *     puts a into its own list), as CSR: out_offsets i32 [n_vertices + 1], out_neighbours i32 with room for 6 n_triangles entries of
 *     which offsets[n_vertices] = *d_count (i32, device) are written.
 * kpx_mesh_non_manifold_edges: the undirected edges {t0,t1}, {t1,t2}, {t2,t0} of every triangle, keyed min << 32 | max; out_edges i32
 *     [3 n_triangles][2] receives, ascending, the (min, max) of the keys that occur more than 2 times (allow_boundary_edges != 0) or a
 *     number of times other than 2 (== 0); *d_count (i32, device) = how many.
 * kpx_mesh_cluster_triangles: triangles that share an edge key are adjacent; out_clusters i32 [n_triangles] = the id of each triangle's
 *     connected component, components numbered by their smallest triangle index; out_n_triangles i32 and out_area f64, each with room
 *     for n_triangles entries of which *d_count (i32, device) are written: the component's triangle count and the sum from 0, in
 *     ascending triangle index, of its triangles' sqrt((nx^2 + ny^2) + nz^2) * 0.5 (n as kpx_mesh_normals').  *d_count = KPX_ERR_RANGE
 *     when a union-find hook gave up.
 * kpx_mesh_flags: out_flags u8 [n_flags].  KPX_MESH_FLAG_REFERENCED: n_flags = n_vertices, 1 where some triangle names the vertex.
 *     KPX_MESH_FLAG_DEGENERATE: n_flags = n_triangles, 1 where two of the triangle's indices are equal.  KPX_MESH_FLAG_INDICES: 1 at
 *     every indices[j] (i64 [n_indices], device) inside [0, n_flags), values outside are ignored.
 * kpx_mesh_select_triangles: the triangles (and their normals when out_triangle_normals is given) with (flags[t] != 0) != (invert != 0),
 *     in order; outputs have room for n_triangles rows, *d_count (i32, device) are written.
 * kpx_mesh_select_vertices: the vertices with (flags[v] != 0) != (invert != 0), in order, with their colours and normals (optional);
 *     the triangles whose three corners stay, in order, renumbered by the rank of their corners, with their normals (optional).
 *     d_counts i32 [2] (device): vertices, triangles written.  ws: kpx_mesh_select_workspace_bytes(n_vertices, n_triangles), for
 *     kpx_mesh_select_triangles (0, n_triangles).
 * kpx_mesh_smooth: `iterations` steps (KPX_MESH_SMOOTH_TAUBIN: pairs of steps, lambda_filter then mu) over the CSR adjacency, on fp64
 *     copies of the arrays whose output is given (out_vertices, out_normals, out_colors; any may be NULL = not filtered), rounded to
 *     float32 once at the end.  x = the vertices at the start of the step (the input's when they are not filtered), y = any filtered
 *     array, u over N(v) ascending.  SIMPLE: y'[v] = (y[v] + sum y[u]) / (1 + |N(v)|).  LAPLACIAN step(l): w = 1 / (sqrt((d0 d0 + d1 d1)
 *     + d2 d2) + 1e-12), d = x[v] - x[u]; y'[v] = y[v] + l (sum w y[u] / sum w - y[v]); |N(v)| = 0 keeps y[v].  One launch per step.
 * kpx_mesh_sample_points: n_points points, ordered by triangle.  prefix_t = the sum from 0 of the areas up to t (as
 *     kpx_mesh_surface_area); upto_t = llround(prefix_t / total * n_points), the last n_points; point p lies in triangle #{upto_t <= p}.
 *     Philox-4x32-10, counter (p lo, p hi, 0x4D534D50, 0), key = seed: r1 = ((w1 << 32 | w0) >> 11) 2^-53, r2 from w3:w2; q = sqrt(r1),
 *     a = 1 - q, b = q (1 - r2), c = q r2; out = (a v0 + b v1) + c v2 as float32, colours (optional) alike, normals (optional) alike
 *     from vertex_normals, else the row of triangle_normals.  *d_total (f64, device) = total; nothing is written unless total > 0. */
#define KPX_MESH_FLAG_REFERENCED 0
#define KPX_MESH_FLAG_DEGENERATE 1
#define KPX_MESH_FLAG_INDICES 2
#define KPX_MESH_SMOOTH_SIMPLE 0
#define KPX_MESH_SMOOTH_LAPLACIAN 1
#define KPX_MESH_SMOOTH_TAUBIN 2
size_t kpx_mesh_adjacency_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_adjacency(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t *out_offsets, int32_t *out_neighbours,
                       int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
size_t kpx_mesh_edges_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_non_manifold_edges(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t allow_boundary_edges,
                                int32_t *out_edges, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
size_t kpx_mesh_cluster_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_cluster_triangles(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, int32_t *out_clusters,
                               int32_t *out_n_triangles, double *out_area, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_mesh_flags(int32_t kind, const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, const int64_t *indices, int64_t n_indices,
                   uint8_t *out_flags, int64_t n_flags, void *stream);
size_t kpx_mesh_select_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_select_triangles(const int32_t *triangles, const float *triangle_normals, int64_t n_triangles, const uint8_t *flags, int32_t invert,
                              int32_t *out_triangles, float *out_triangle_normals, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_mesh_select_vertices(const float *vertices, const float *colors, const float *normals, int64_t n_vertices, const int32_t *triangles,
                             const float *triangle_normals, int64_t n_triangles, const uint8_t *flags, int32_t invert, float *out_vertices,
                             float *out_colors, float *out_normals, int32_t *out_triangles, float *out_triangle_normals, int32_t *d_counts, void *ws,
                             size_t ws_bytes, void *stream);
size_t kpx_mesh_smooth_workspace_bytes(int64_t n_vertices);
int kpx_mesh_smooth(const float *vertices, const float *normals, const float *colors, int64_t n_vertices, const int32_t *offsets,
                    const int32_t *neighbours, int64_t n_neighbours, int32_t method, int32_t iterations, double lambda_filter, double mu,
                    float *out_vertices, float *out_normals, float *out_colors, void *ws, size_t ws_bytes, void *stream);
size_t kpx_mesh_sample_workspace_bytes(int64_t n_triangles);
int kpx_mesh_sample_points(const float *vertices, const float *colors, const float *vertex_normals, const float *triangle_normals,
                           int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, int64_t n_points, uint64_t seed, float *out_points,
                           float *out_colors, float *out_normals, double *d_total, void *ws, size_t ws_bytes, void *stream);

/* ---- ray casts and closest points on triangle meshes ([O3D] t.geometry.RaycastingScene; arithmetic contract AC14) --
 * A scene is a caller-owned device buffer of kpx_rayscene_bytes(n_triangles) bytes that kpx_rayscene_build fills from float32 vertices
 * [n_vertices][3] and int32 triangles [n_triangles][3] (the geometries of a scene concatenated, indices into the concatenated vertices;
 * every index must lie in [0, n_vertices) and every coordinate must be finite: the caller checks): header, the boxes of an implicit
 * complete tree (leaves of KPX_RAYSCENE_LEAF triangles consecutive along a space-filling curve, KPX_RAYSCENE_FANOUT children per node),
 * the corners and ids of the triangles.  triangle_ids (i32 [n_triangles][2], optional): the geometry id and primitive id reported for
 * each triangle; NULL: geometry 0, primitive = the triangle's index.  The scene does not point back into the mesh and the library keeps
 * no state.  At most 2^28 triangles (the size queries return 0 beyond).  ws: kpx_rayscene_workspace_bytes(n_triangles).  Asynchronous.
 * kpx_rayscene_rays: rays f32 [m][6] = origin, direction (not normalised: t is in units of |d|).  All arithmetic fp64, every multiply
 *     and add separate.  Triangle (v0, v1, v2): e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1.p (0: miss), inv = 1 / det, s = o - v0,
 *     u = (s.p) inv, q = s x e1, v = (d.q) inv, t = (e2.q) inv; a hit needs u >= 0, v >= 0, u + v <= 1, the ray to meet the triangle's box
 *     (corner min / max widened by 2^-20 of the largest coordinate magnitude; slab test from tn = 0, tf = +inf) and tn <= t <= tf.  A ray
 *     with a non-finite component or a zero direction hits nothing.
 *     KPX_RAY_CAST: the hit of the smallest t, ties to the lowest triangle index: out_t f64 [m] (+inf: miss), out_t_hit f32 [m],
 *         out_uvs f32 [m][2], out_normals f32 [m][3] (kpx_mesh_normals' normalised normal; a miss: zeros), the two ids i32 [m] (-1: miss).
 *     KPX_RAY_OCCLUDED: out_count i32 [m] = 1 when some hit has tnear <= t <= tfar, else 0.
 *     KPX_RAY_COUNT: out_count = the number of triangles hit (a ray through a shared edge counts both).
 *     Outputs a mode does not write may be NULL.
 * kpx_rayscene_closest: queries f32 [m][3].  Per triangle Ericson's closest point (regions A, B, AB, C, AC, BC, interior) and
 *     D = max(d2(q, closest) as AC3, gap2 of the triangle's box); the smallest D wins, ties to the lowest triangle index, a NaN D never
 *     wins.  out_d2 f64 [m] = D, out_points f32 [m][3], out_distance f32 [m] = (float)sqrt(D), ids i32 [m].  A query with a non-finite
 *     coordinate gets NaN and -1.  A scene without triangles is KPX_ERR_INVALID.
 * brute != 0: every triangle is tested in ascending index instead of walking the tree; results are the same bits (second witness and
 * yardstick).  Every query call reads the scene header back (one small copy and a synchronisation of `stream`) and rejects a buffer
 * that is not a scene or is smaller than the scene it claims to be. */
#define KPX_RAYSCENE_LEAF 4
#define KPX_RAYSCENE_FANOUT 4
#define KPX_RAY_CAST 0
#define KPX_RAY_OCCLUDED 1
#define KPX_RAY_COUNT 2
size_t kpx_rayscene_bytes(int64_t n_triangles);
size_t kpx_rayscene_workspace_bytes(int64_t n_triangles);
int kpx_rayscene_build(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, const int32_t *triangle_ids,
                       void *scene, size_t scene_bytes, void *ws, size_t ws_bytes, void *stream);
int kpx_rayscene_rays(const void *scene, size_t scene_bytes, const float *rays, int64_t m, int32_t mode, double tnear, double tfar, int32_t brute,
                      double *out_t, float *out_t_hit, float *out_uvs, float *out_normals, int32_t *out_geometry_ids, int32_t *out_primitive_ids,
                      int32_t *out_count, void *stream);
int kpx_rayscene_closest(const void *scene, size_t scene_bytes, const float *queries, int64_t m, int32_t brute, double *out_d2, float *out_points,
                         float *out_distance, int32_t *out_geometry_ids, int32_t *out_primitive_ids, void *stream);

/* ---- mesh checks ([O3D] geometry.TriangleMesh; arithmetic contract AC15) ---------------------------------------------
 * Arrays, index rule, limits and fp64 arithmetic as in the clean-up section above; tests/mesh_checks_ref.py is the pinned statement.
 * kpx_mesh_non_manifold_vertices: the link of v has one edge {u, w} per triangle in which v occurs exactly once (u, w: its other two
 *     corners); out_vertices i32 (room for n_vertices) receives, ascending, the vertices whose link has more than one connected
 *     component, *d_count (i32, device) = how many, or KPX_ERR_RANGE when a union-find hook gave up.  A vertex without a link edge is not
 *     reported.  ws: kpx_mesh_links_workspace_bytes.
 * kpx_mesh_orientation: triangles with a repeated index take no part.  Two others are neighbours when they share an edge key (every pair
 *     of a run of equal keys) and agree on it when they run it in opposite directions.  *d_orientable (i32, device) = 1 when some flip
 *     assignment makes all neighbours agree on all shared edges, 0 when none does, KPX_ERR_RANGE when a hook gave up.  When orientable:
 *     in every connected component the smallest triangle keeps its winding and decides the rest; out_flip u8 [n_triangles] (optional) =
 *     1 for the triangles to flip, apply_triangles (optional, may be `triangles` itself) gets (t0, t1, t2) -> (t0, t2, t1) for them and
 *     apply_triangle_normals (optional) their rows negated.  When not orientable out_flip is 0 and nothing else is written.
 * kpx_mesh_volume: *d_volume (f64, device) = |S| / 6.0, S the sum from 0, in ascending triangle index, of v0 . (v1 x v2) (cross
 *     components a b - c d, dot (x x' + y y') + z z').  Whether the mesh encloses a volume is the caller's question.
 * kpx_mesh_edge_count: *d_count (i32, device) = the number of distinct edge keys.  ws: kpx_mesh_edges_workspace_bytes.
 * kpx_rayscene_triangle_pairs_*: one query triangle per row of `triangles` (indices into `vertices`) against the triangles of a scene.
 *     A query i and a scene triangle g intersect when their exact boxes (corner min / max as doubles, no padding; closed comparison)
 *     overlap and Moeller's division-free interval test with the coplanar fallback, tri_tri(i, g) of the pinned statement, says so
 *     (plane distances below the absolute 1e-6 count as 0).  self != 0: the queries are the very triangles the scene was built from
 *     (m = its triangle count, else KPX_ERR_INVALID); only g > i is examined and a pair that shares a vertex index is skipped.
 *     _count, any == 0: out_offsets i64 [m + 1] = the exclusive prefix sums of the queries' partner counts, [m] the total.
 *     _count, any != 0: *d_flag (i32, device) = 1 when some query has a partner, else 0; lanes stop at their first.
 *     _fill: out_pairs i32 [n_pairs][2] = the pairs (i, g) ascending in (i, g); offsets and n_pairs as _count left them (the caller reads
 *         offsets[m]); more than 2^31 - 1 pairs is KPX_ERR_RANGE.  ws: kpx_rayscene_triangle_pairs_workspace_bytes(n_pairs).
 *     brute != 0: every scene triangle in ascending index instead of the tree walk; same pairs.  The tree prunes a node only when its
 *     box does not overlap the query's exact box.  Scene checks and the header read-back as for the ray queries. */
size_t kpx_mesh_links_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_non_manifold_vertices(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t *out_vertices, int32_t *d_count, void *ws,
                                   size_t ws_bytes, void *stream);
size_t kpx_mesh_orientation_workspace_bytes(int64_t n_vertices, int64_t n_triangles);
int kpx_mesh_orientation(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, uint8_t *out_flip, int32_t *apply_triangles,
                         float *apply_triangle_normals, int32_t *d_orientable, void *ws, size_t ws_bytes, void *stream);
size_t kpx_mesh_volume_workspace_bytes(int64_t n_triangles);
int kpx_mesh_volume(const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double *d_volume, void *ws,
                    size_t ws_bytes, void *stream);
int kpx_mesh_edge_count(const int32_t *triangles, int64_t n_vertices, int64_t n_triangles, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_rayscene_triangle_pairs_count(const void *scene, size_t scene_bytes, const float *vertices, int64_t n_vertices, const int32_t *triangles,
                                      int64_t m, int32_t self, int32_t any, int32_t brute, int64_t *out_offsets, int32_t *d_flag, void *stream);
size_t kpx_rayscene_triangle_pairs_workspace_bytes(int64_t n_pairs);
int kpx_rayscene_triangle_pairs_fill(const void *scene, size_t scene_bytes, const float *vertices, int64_t n_vertices, const int32_t *triangles,
                                     int64_t m, int32_t self, int32_t brute, const int64_t *offsets, int64_t n_pairs, int32_t *out_pairs, void *ws,
                                     size_t ws_bytes, void *stream);

/* ---- occupancy grids ([O3D] geometry.VoxelGrid; arithmetic contract AC10) ---------------------------------------- */
/* A grid is caller-owned: keys u64 [M], strictly ascending, key = gx << 42 | gy << 21 | gz with every index in [0, 2^21), and colors
 * f32 [M][3]; voxel g covers h_origin + g voxel .. h_origin + (g + 1) voxel.  All decisions are fp64.
 * kpx_voxelgrid_from_cloud: the grid of a float32 cloud (create_from_point_cloud: h_origin NULL, origin = min_bound - voxel / 2;
 *     create_from_point_cloud_within_bounds: h_origin = the caller's min_bound, host).  g = floor((p - origin) / voxel); the colour of a
 *     voxel is (float)(sum / count) of its points' colours, summed in fp64 in ascending point index (col NULL: zeros).  keys and colors
 *     hold up to n rows; d_origin (f64 [3], device) receives the origin, d_count (i32, device) the number of voxels, or KPX_ERR_RANGE
 *     when an index leaves [0, 2^21) (Open3D's "voxel_size is too small").  Asynchronous.
 * kpx_voxelgrid_dense: all nw nh nd indices, ascending (gx, gy, gz), every voxel with h_color (host f32 [3]).  Every dimension
 *     <= KPX_VOXELGRID_AXIS_CELLS, at most 2^31 - 1 voxels.  Asynchronous.
 * kpx_voxelgrid_carve: carve_depth_map (mode KPX_VOXELGRID_DEPTH) / carve_silhouette (KPX_VOXELGRID_SILHOUETTE) with `count` images of
 *     width x height >= 2 x 2 pixels taken with the pinhole h_intrinsic = (fx, fy, cx, cy) from h_extrinsics f64 [count][16] (world ->
 *     camera, row-major, host).  A voxel survives an image when one of its 8 corners keeps it -- a corner projects to (u, v, z), WITHOUT
 *     a test of the sign of z; outside the image it keeps iff keep_voxels_outside_image; inside, with d the bilinear sample of the image
 *     there, it keeps iff d > 0 and (silhouette, or z >= d), and with keep_unmeasured also when !(d > 0) -- and it survives the call
 *     when it survives every image: the result equals `count` calls with one image each, in any order.  One launch holds up to
 *     KPX_VOXELGRID_MAX_IMAGES images, larger counts run as consecutive launches.  h_images: host array of device pointers [H W] of
 *     `format`: KPX_VOXELGRID_F32 (depth_scale, depth_trunc ignored), KPX_VOXELGRID_U16 (d = (float)raw / (float)depth_scale,
 *     d > (float)depth_trunc -> 0, as kpx_tsdf_integrate) or KPX_VOXELGRID_U8 (a mask: nonzero = 1).  Survivors go to out_keys /
 *     out_colors (room for m rows; they must not alias the input) in their order, their number to d_count (i32, device).  Asynchronous.
 * kpx_voxelgrid_included: out[i] = 1 iff query i (f32 [n][3], or f64 when queries_f64) lies in a voxel of the grid: g = floor((q -
 *     origin) / voxel), every component in [0, 2^21) (NaN: not included), key present.  Asynchronous. */
#define KPX_VOXELGRID_AXIS_CELLS 2097152
#define KPX_VOXELGRID_MAX_IMAGES 8
#define KPX_VOXELGRID_DEPTH 0
#define KPX_VOXELGRID_SILHOUETTE 1
#define KPX_VOXELGRID_F32 0
#define KPX_VOXELGRID_U16 1
#define KPX_VOXELGRID_U8 2
size_t kpx_voxelgrid_from_cloud_workspace_bytes(int64_t n);
int kpx_voxelgrid_from_cloud(const float *pts, const float *col, int64_t n, double voxel, const double *h_origin, uint64_t *keys, float *colors,
                             double *d_origin, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_voxelgrid_dense(int32_t nw, int32_t nh, int32_t nd, const float *h_color, uint64_t *keys, float *colors, void *stream);
size_t kpx_voxelgrid_carve_workspace_bytes(int64_t m);
int kpx_voxelgrid_carve(const uint64_t *keys, const float *colors, int64_t m, const double *h_origin, double voxel, int32_t mode, int32_t count,
                        const void *const *h_images, int32_t format, double depth_scale, double depth_trunc, int32_t width, int32_t height,
                        const double *h_intrinsic, const double *h_extrinsics, int32_t keep_voxels_outside_image, int32_t keep_unmeasured,
                        uint64_t *out_keys, float *out_colors, int32_t *d_count, void *ws, size_t ws_bytes, void *stream);
int kpx_voxelgrid_included(const void *queries, int32_t queries_f64, int64_t n, const uint64_t *keys, int64_t m, const double *h_origin, double voxel,
                           uint8_t *out, void *stream);

/* ---- image operators and RGB-D odometry ([O3D] geometry.Image filters / pyramids, pipelines.odometry; arithmetic contract AC11,
 *      DESIGN.md 3 / 5.13) -------------------------------------------------------------------------------------------------------- */
/* Images are f32 [count][height][width], row-major, caller-owned, on the device; h_intrinsic = (fx, fy, cx, cy), host.
 * kpx_image_filter: the separable filters of Open3D's Image::Filter: a horizontal pass, then a vertical pass; taps outside the image
 *     read the border pixel; every output is accumulated in fp64 over the taps in ascending order and rounded to f32 once per pass.
 *     GAUSSIAN3 (.25 .5 .25), GAUSSIAN5 (.0625 .25 .375 .25 .0625), GAUSSIAN7 (.03125 .109375 .21875 .28125 .21875 .109375 .03125),
 *     SOBEL3DX ((-1 0 1) along x, (1 2 1) along y), SOBEL3DY (its transpose).  dst must not alias src.  ws: kpx_image_workspace_bytes.
 * kpx_image_downsample: dst [count][height / 2][width / 2], every pixel the f32 (((a + b) + c) + d) / 4 of its 2 x 2 block (a b the
 *     upper row).  width, height >= 2.
 * kpx_odometry_correspondence: AC11's correspondences of one pair of depth images (NaN = no measurement) under h_extrinsic (row-major
 *     4x4, host): source pixel (u_s, v_s) with finite depth d: q = d (K R K^-1) (u_s, v_s, 1) + K t, z' = q_z > 0, u_t = (int)(q_x / z' +
 *     0.5), v_t likewise (truncation), inside the target, the target depth d_t there finite, |z' - d_t| <= depth_diff_max; a target
 *     pixel keeps the source of the smallest (float)z', equal ones the smallest v_s W + u_s.  corres: i32 [width height][4] rows
 *     (u_s, v_s, u_t, v_t) ascending in (v_t, u_t); d_count: i32, device.
 * kpx_rgbd_odometry: compute_rgbd_odometry for `pairs` pairs in one chain of launches (pair = grid.y), no host read-back inside.
 *     raw = 0: depth_* / color_* are f32 [pairs][H W] (depth, intensity); raw = 1: depth_* u16 [pairs][H W], color_* u8 [pairs][H W][3],
 *     converted as RGBDImage.create_from_color_and_depth does (d = (float)raw / (float)depth_scale, d > (float)depth_trunc -> 0,
 *     intensity = ((0.299f r + 0.587f g) + 0.114f b) / 255f); mask_* (u8 [pairs][H W] or NULL, raw = 1 only): nonzero = depth 0.
 *     h_init f64 [pairs][16]; jacobian KPX_ODOMETRY_COLOR / KPX_ODOMETRY_HYBRID; h_iterations i32 [levels], index 0 = the coarsest
 *     level.  d_results f64 [pairs][KPX_ODOMETRY_RESULT_DOUBLES], device: [0] success (1 / 0), [1] correspondences behind the
 *     information matrix, [2..17] the 4x4, [18..53] the 6x6 information matrix (both the identity on failure).
 * kpx_odometry_iteration: ONE Gauss-Newton step of AC11 at one pyramid level, given that level's eight images (source / target
 *     intensity and depth, the target's Sobel images) and camera.  d_out f64 [KPX_ODOMETRY_ITERATION_DOUBLES], device: [0..20] the
 *     upper triangle of J^T J by rows, [21..26] J^T r, [27] r.r, [28] the number of correspondences, [29] 1 = solved (0 = singular or
 *     no correspondence), [30..45] the updated 4x4 (the given one when not solved).
 * All asynchronous; ws: kpx_odometry_workspace_bytes(pairs, width, height, levels) (1, ..., 1 for the two single-pair calls). */
#define KPX_IMAGE_GAUSSIAN3 0
#define KPX_IMAGE_GAUSSIAN5 1
#define KPX_IMAGE_GAUSSIAN7 2
#define KPX_IMAGE_SOBEL3DX 3
#define KPX_IMAGE_SOBEL3DY 4
#define KPX_ODOMETRY_COLOR 0
#define KPX_ODOMETRY_HYBRID 1
#define KPX_ODOMETRY_MAX_LEVELS 8
#define KPX_ODOMETRY_RESULT_DOUBLES 54
#define KPX_ODOMETRY_ITERATION_DOUBLES 46
size_t kpx_image_workspace_bytes(int32_t count, int32_t width, int32_t height);
int kpx_image_filter(const float *src, float *dst, int32_t count, int32_t width, int32_t height, int32_t filter_type, void *ws, size_t ws_bytes,
                     void *stream);
int kpx_image_downsample(const float *src, float *dst, int32_t count, int32_t width, int32_t height, void *stream);
size_t kpx_odometry_workspace_bytes(int32_t pairs, int32_t width, int32_t height, int32_t levels);
int kpx_odometry_correspondence(const float *depth_s, const float *depth_t, int32_t width, int32_t height, const double *h_intrinsic,
                                const double *h_extrinsic, double depth_diff_max, int32_t *corres, int32_t *d_count, void *ws, size_t ws_bytes,
                                void *stream);
int kpx_rgbd_odometry(int32_t pairs, const void *depth_s, const void *color_s, const void *depth_t, const void *color_t, int32_t raw,
                      const uint8_t *mask_s, const uint8_t *mask_t, double depth_scale, double depth_trunc, int32_t width, int32_t height,
                      const double *h_intrinsic, const double *h_init, int32_t jacobian, int32_t levels, const int32_t *h_iterations,
                      double depth_diff_max, double depth_min, double depth_max, double *d_results, void *ws, size_t ws_bytes, void *stream);
int kpx_odometry_iteration(const float *color_s, const float *depth_s, const float *color_t, const float *depth_t, const float *color_dx,
                           const float *color_dy, const float *depth_dx, const float *depth_dy, int32_t width, int32_t height,
                           const double *h_intrinsic, const double *h_extrinsic, int32_t jacobian, double depth_diff_max, double *d_out, void *ws,
                           size_t ws_bytes, void *stream);

/* ---- normal orientation (arithmetic contract AC17) ------------------------------------------------------------------
 * pts, normals: f32 [n][3] on the device; the normals are rewritten in place.  All decision arithmetic is fp64 on the f32 values,
 * every multiply and add rounded separately: dot(a, b) = (ax bx + ay by) + az bz, len = sqrt(dot(n, n)); a flip negates the three
 * components.  n >= 2^31 is KPX_ERR_RANGE; null pointers, an unknown mode and k outside [0, KPX_ORIENT_MAX_K] are rejected before the
 * device is touched; n = 0 does nothing.
 * kpx_orient_normals (one streaming kernel, asynchronous), h_ref f64 [3] on the host:
 *     KPX_ORIENT_NORMALIZE: len > 0: every component becomes (float)(c / len).  pts and h_ref are not read (may be NULL).
 *     KPX_ORIENT_DIRECTION: len == 0: the normal becomes (float)h_ref; else flipped when dot(n, h_ref) < 0.  pts is not read.
 *     KPX_ORIENT_CAMERA: r = h_ref - p; len == 0: the normal becomes (float)(r / |r|), (0, 0, 1) when |r| == 0; else flipped when
 *         dot(n, r) < 0.
 * kpx_emst: the Euclidean minimum spanning tree of the cloud: the unique minimum spanning tree of the complete graph whose pairs
 *     {a < b} are ordered by (d2(a, b), a, b), d2 the squared distance of kpx_search_knn.  edges: i32 [n - 1][2], rows (a < b) ascending
 *     in (a, b).  k is the width of the neighbour lists the Boruvka rounds work from: it changes the time, never the result.
 * kpx_orient_normals_tangent: [O3D] OrientNormalsConsistentTangentPlane(k) with its ties pinned.  Graph: the tree of kpx_emst plus
 *     {v, u} for every u != v among the first min(k, n) entries of v's kpx_search_knn row of the cloud queried with itself; weights
 *     w(a, b) = 1 - |dot(n_a, n_b)| on the input normals; T = the unique minimum spanning tree under (w, a, b).  Root r = the lowest
 *     index among the points of maximal z, flipped when n_r.z < 0; along every edge of T from parent a to child b, c = dot(n_a, n_b)
 *     of the input normals: c == 0 leaves b as it came in, otherwise b is flipped when (a is flipped) != (c < 0).  flips (u8 [n], 1 =
 *     negated) and tree (i32 [n - 1][2], T's rows (a < b) ascending in (a, b)) are optional (NULL).  Its EMST works from rows of
 *     max(k, 30) entries whatever k is (the tree does not depend on that width, the time does); the graph takes the first min(k, n).
 * h_stats (i64 [8] on the host, or NULL): [0] rounds of the EMST, [1] points that took the bounded exact search (summed over the
 *     rounds), [2] the unbounded one, [3] rounds of T, [4] edges of T with c == 0 (more than none: the signs are walked on the host).
 * kpx_emst and kpx_orient_normals_tangent read one word back per round: they return with the stream drained. */
#define KPX_ORIENT_NORMALIZE 0
#define KPX_ORIENT_DIRECTION 1
#define KPX_ORIENT_CAMERA 2
#define KPX_ORIENT_MAX_K 4096
int kpx_orient_normals(const float *pts, float *normals, int64_t n, int32_t mode, const double *h_ref, void *stream);
size_t kpx_emst_workspace_bytes(int64_t n, int32_t k);
int kpx_emst(const float *pts, int64_t n, int32_t k, int32_t *edges, int64_t *h_stats, void *ws, size_t ws_bytes, void *stream);
size_t kpx_orient_normals_tangent_workspace_bytes(int64_t n, int32_t k);
int kpx_orient_normals_tangent(const float *pts, float *normals, int64_t n, int32_t k, uint8_t *flips, int32_t *tree, int64_t *h_stats, void *ws,
                               size_t ws_bytes, void *stream);

/* ---- PointNet joint regression, inference (arithmetic contract AC18) ---------------------------------------------------
 * models/pointnet.py create_pointnet(number_of_points, number_of_joints) with batch normalisation on its moving statistics (folded
 * into the layer in front of it) and dropout as the identity; evaluate.py's metrics.
 * The model is 20 layers (W f32 [c_in][c_out] row-major, b f32 [c_out]), y = x W + b, ReLU after every layer except the three marked *:
 *    0..5   tnet(3):   3 -> 32, 32 -> 64, 64 -> 512, max over the points, 512 -> 256, 256 -> 128, 128 -> 9 *
 *    6..7              3 -> 32, 32 -> 32                                        (applied to x T3,  T3[k][j] = t[3 k + j])
 *    8..13  tnet(32):  32 -> 32, 32 -> 64, 64 -> 512, max, 512 -> 256, 256 -> 128, 128 -> 1024 *
 *    14..19            32 -> 32, 32 -> 64, 64 -> 512, max, 512 -> 256, 256 -> 128, 128 -> 3 joints *      (applied to f T32)
 * weights: the packed buffer, f32, 16-byte aligned: for layer 0, 1, ... its W then its b, each array starting at a multiple of 64
 *     floats (gaps are not read).  W is stored [c_in][c_out] row-major, except for the three 64 -> 512 layers (2, 10, 16), which are
 *     stored in the operand order of v_mfma_f32_32x32x2_f32: element ((c 8 + q) 64 + l) 4 + e = W[2 (4 q + e) + (l >> 5)][32 c + (l & 31)],
 *     c < 16, q < 8, l < 64, e < 4.  weights_floats: the length of the buffer, checked against the layout for `joints`.
 * pts: f32 [batch][n][3]; out: f32 [batch][3 joints].  Optional stage outputs (NULL = not wanted): T3 f32 [batch][9], T32 f32
 *     [batch][1024], g1 / g2 / g3 f32 [batch][512] (the three maxima over the points).
 * Arithmetic: f32 products and sums, fused multiply-adds, in an order that is fixed for a cloud whatever the batch around it; the maxima
 *     are exact (integer atomicMax on the bit patterns of values >= +0), so a result does not depend on scheduling.  relu(x) = x > 0 ? x
 *     : +0.  Non-finite coordinates give an unspecified result.
 * joints >= 1 and 3 joints <= KPX_POINTNET_MAX_OUT; n = 0 is rejected; batch n >= 2^31 is KPX_ERR_RANGE; batch = 0 does nothing.  All
 *     arguments are checked before the device is touched.  Six launches and the clears of the maxima, asynchronous, no host read-back.
 * kpx_joint_metrics: over the n = batch 3 joints values of y_true, y_pred (f32): d_counts[t] (i64, device) = the number of
 *     |(float)(pred - true)| <= (float)h_thresholds[t] (metrics/metric.py's float32 comparison; h_thresholds f64 on the host,
 *     n_thresholds <= KPX_METRICS_MAX_THRESHOLDS), d_sum_sq (f64, device) = the sum of the squared f32 differences, each squared and
 *     added in fp64 in a fixed order.  Asynchronous. */
#define KPX_POINTNET_MAX_OUT 1024
#define KPX_METRICS_MAX_THRESHOLDS 64
size_t kpx_pointnet_workspace_bytes(int32_t batch, int64_t n, int32_t joints);
int kpx_pointnet_forward(const float *weights, int64_t weights_floats, const float *pts, int32_t batch, int64_t n, int32_t joints, float *out,
                         float *T3, float *T32, float *g1, float *g2, float *g3, void *ws, size_t ws_bytes, void *stream);
int kpx_joint_metrics(const float *y_true, const float *y_pred, int64_t n, const double *h_thresholds, int32_t n_thresholds, int64_t *d_counts,
                      double *d_sum_sq, void *stream);

/* ---- PointNet joint regression, training (arithmetic contract AC19) ------------------------------------------------------
 * One step of train.py's model.fit on create_pointnet: batch normalisation on the batch statistics (epsilon 1e-3, momentum 0: the moving
 * statistics become the step's batch statistics), Dropout(0.3) behind the two main-head dense_bn blocks, loss = the mean squared error
 * plus the two OrthogonalRegularizer terms divided by the batch size, gradients of the 74 trainable arrays, Adam.
 * params: the parameter buffer, f32, 16-byte aligned, every array starting at a multiple of 64 floats (gaps are zero and stay zero):
 *     the TRAINABLE part first -- for layer 0, 1, ..., 19 (numbered as above) its kernel [c_in][c_out] row-major, its bias [c_out] and,
 *     for the 17 layers with batch normalisation (all but 5, 13, 19), gamma [c_out] and beta [c_out] -- then, for the same 17 layers in
 *     order, moving_mean [c_out] and moving_variance [c_out].  kpx_pointnet_train_floats gives the length of the buffer (*total) and of its
 *     trainable part (*trainable); grad, m and v have the trainable part's layout.
 * kpx_pointnet_grad: x f32 [batch][n][3], y f32 [batch][3 joints] -> loss f32 [3] on the device (total, mean squared error,
 *     regulariser), grad, and the moving statistics written into params.  training_dropout 0 leaves dropout out; otherwise the element
 *     (row, channel) of dropout layer d (0: behind 512 -> 256, 1: behind 256 -> 128) is kept iff (h >> 8) < 11744051 with
 *     h = mix(mix(mix(mix(seed) ^ step) ^ d) ^ (512 row + channel)) in 32-bit arithmetic (seed and step taken modulo 2^32),
 *     mix(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16; kept values are multiplied by fl32(1 / 0.7).
 *     Optional stage outputs (NULL = not wanted): T3 [batch][9], T32 [batch][1024], g1 / g2 / g3 f32 [batch][512] the pooled
 *     activations with i1 / i2 / i3 i32 [batch][512] the pooled points, out [batch][3 joints].  The pooled point of (cloud, channel) is the
 *     one with the largest sign(gamma) z, the lowest index among equal z; where the pooled activation is 0 (no gradient) index 0.
 * kpx_adam_step: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps), t >= 1,
 *     evaluated in fp64 on the f32 inputs, each stored value rounded once.  One launch.
 * kpx_pointnet_train_step: kpx_pointnet_grad, then kpx_adam_step over the trainable part; the same bits as the two calls.
 * Arithmetic: f32 storage, f32 products and fused multiply-adds in the point-wise layers; every sum over points or rows is per-block
 *     partial sums in a fixed order, combined in ascending order in fp64, and the B-row sums of the heads are taken in fp64; no
 *     floating-point atomics: two runs give the same bits, whatever the workspace held.  joints, n and batch are checked as for kpx_pointnet_forward, the buffer
 *     length and the workspace size before the device is touched; batch = 0 clears loss and grad and does nothing else.
 *     Asynchronous on `stream`, no host read-back. */
int kpx_pointnet_train_floats(int32_t joints, int64_t *total, int64_t *trainable);
size_t kpx_pointnet_train_workspace_bytes(int32_t batch, int64_t n, int32_t joints);
int kpx_pointnet_grad(float *params, int64_t params_floats, const float *x, const float *y, int32_t batch, int64_t n, int32_t joints, uint64_t seed,
                      uint64_t step, int32_t training_dropout, float *loss, float *grad, float *T3, float *T32, float *g1, int32_t *i1, float *g2,
                      int32_t *i2, float *g3, int32_t *i3, float *out, void *ws, size_t ws_bytes, void *stream);
int kpx_adam_step(float *w, const float *g, float *m, float *v, int64_t count, double lr, double beta1, double beta2, double eps, int64_t t,
                  void *stream);
int kpx_pointnet_train_step(float *params, int64_t params_floats, const float *x, const float *y, int32_t batch, int64_t n, int32_t joints,
                            uint64_t seed, uint64_t step, int32_t training_dropout, float *loss, float *grad, float *m, float *v, double lr,
                            double beta1, double beta2, double eps, int64_t t, void *ws, size_t ws_bytes, void *stream);

/* ---- sensor calibration: lens-model ray tables, colour aligned to depth (arithmetic contract AC20) ---------------------
 * A camera is KPX_CAMERA_DOUBLES doubles on the host: fx, fy, cx, cy, k1, k2, k3, k4, k5, k6, p1, p2, metric_radius (pixel units,
 * integer pixel coordinates are pixel centres, OpenCV's rational model).  Everything below is fp64, every multiply, add and divide
 * rounded separately, in exactly the order written here (no fused multiply-add anywhere):
 *   distort(x, y):  xx = x x, yy = y y, r2 = xx + yy, r4 = r2 r2, r6 = r4 r2,
 *                   num = ((1 + k1 r2) + k2 r4) + k3 r6, den = ((1 + k4 r2) + k5 r4) + k6 r6, radial = num / den, xy2 = 2 (x y),
 *                   xd = (x radial + p1 xy2) + p2 (r2 + 2 xx), yd = (y radial + p1 (r2 + 2 yy)) + p2 xy2.
 *   forward(X, Y, Z), Z > 0:  x = X / Z, y = Y / Z; invalid when r2 > metric_radius metric_radius; u = fx xd + cx, v = fy yd + cy.
 *   jacobian(x, y): nd = (k1 + (2 k2) r2) + (3 k3) r4, dd = (k4 + (2 k5) r2) + (3 k6) r4, dr = (nd den - num dd) / (den den),
 *                   gx = (2 x) dr, gy = (2 y) dr,
 *                   a = ((radial + x gx) + (2 p1) y) + (6 p2) x,   b = (x gy + (2 p1) x) + (2 p2) y,
 *                   c = (y gx + (2 p1) x) + (2 p2) y,              d = ((radial + y gy) + (6 p1) y) + (2 p2) x.
 *   inverse(u, v):  xn = (u - cx) / fx, yn = (v - cy) / fy, (x, y) = (xn, yn); then up to 21 rounds: (xd, yd) = distort(x, y),
 *                   ex = xd - xn, ey = yd - yn; converged when ex ex + ey ey <= 1e-22 (a NaN never is); the 21st round only tests;
 *                   otherwise det = a d - b c, stop unless det is finite and non-zero,
 *                   x = x - (d ex - b ey) / det, y = y - (a ey - c ex) / det   (at most 20 Newton steps).
 *                   The result is (NaN, NaN) unless converged with x, y finite and x x + y y <= metric_radius metric_radius.
 * kpx_xy_table: xy f32 [height][width][2] on the device = inverse(column, row) rounded once to float32 (NaN pairs where invalid):
 *     the table kpx_unproject_u16 / kpx_depth_to_cloud take.  One thread per pixel, one launch, asynchronous.
 * kpx_color_to_depth: the colour image (or a mask / label image on the colour camera) resampled into the depth camera's pixel grid.
 *     depth u16 [frames][n_px] millimetres; xy f32 [calibrations][n_px][2]; color u8 [frames][color_height][color_width][channels],
 *     channels 1 or 3; out u8 [frames][n_px][channels]; all on the device, no alignment required.  h_calibrations: `calibrations`
 *     (1 .. KPX_SENSOR_MAX_CALIBRATIONS) blocks of KPX_CALIBRATION_DOUBLES doubles on the host: the colour camera, then the row-major
 *     4x4 depth -> colour transform in millimetres (its last row is not read).  Frame f uses calibration f mod calibrations, which
 *     must divide frames.  Per depth pixel with depth d and table entry (xt, yt):
 *         px = xt d, py = yt d, pz = d;   q_i = ((R_i0 px + R_i1 py) + R_i2 pz) + t_i;   (uc, vc) = forward(q) of the colour camera;
 *         KPX_SAMPLE_NEAREST:  the pixel (floor(uc + 0.5), floor(vc + 0.5));
 *         KPX_SAMPLE_BILINEAR: x0 = floor(uc), y0 = floor(vc), ax = uc - x0, ay = vc - y0, per channel
 *             val = (((1 - ax)(1 - ay) c00 + ax (1 - ay) c10) + (1 - ax) ay c01) + ax ay c11 (c10 right of c00, c01 below it),
 *             stored as floor(val + 0.5).
 *     The pixel is all zeros when d == 0, the table entry has a NaN, q_z <= 0, the projection is invalid, the nearest pixel lies
 *     outside the image, or (bilinear) any of the four neighbours does, whatever its weight.  Every output byte is written.  Like the
 *     sensor SDK's own transformation this does not test occlusion between the two cameras.  One launch for the whole batch
 *     (frames <= 65535), asynchronous.
 * Neither entry takes device scratch.  Sizes, null pointers, channels, the sampling code and calibrations not dividing frames are
 * rejected before the device is touched; width height = 0, frames = 0 and n_px = 0 return KPX_OK without a launch. */
#define KPX_CAMERA_DOUBLES 13
#define KPX_CALIBRATION_DOUBLES 29
#define KPX_SENSOR_MAX_CALIBRATIONS 16
#define KPX_SAMPLE_NEAREST 0
#define KPX_SAMPLE_BILINEAR 1
int kpx_xy_table(const double *h_camera, int32_t width, int32_t height, float *xy, void *stream);
int kpx_color_to_depth(const uint16_t *depth, const float *xy, const uint8_t *color, int64_t n_px, int32_t frames, int32_t color_width,
                       int32_t color_height, int32_t channels, const double *h_calibrations, int32_t calibrations, int32_t interpolation,
                       uint8_t *out, void *stream);

/* ---- depth warped into the colour camera, occlusion-tested registration (arithmetic contract AC21) -------------------
 * AC20's rules hold: fp64, every multiply, add and divide rounded separately in the order written, no fused multiply-add.
 *   Vertex of depth pixel (column c, row r) of frame f, calibration f mod calibrations: d the u16 depth, (xt, yt) the table entry;
 *       px = xt d, py = yt d, pz = d;   q_i = ((R_i0 px + R_i1 py) + R_i2 pz) + t_i;   (u, v) = forward(q) of the colour camera, z = q_z
 *       (AC20's "colour -> depth" chain: the same code, the same bits).  The vertex is valid when d != 0, neither table value is NaN,
 *       q_z > 0 and the projection lies inside the metric radius.
 *   Triangles: every 2 x 2 block of depth pixels with top-left (c, r), c < W - 1, r < H - 1, gives, in this vertex order,
 *       A = (P(c, r), P(c + 1, r), P(c, r + 1))   and   B = (P(c + 1, r + 1), P(c, r + 1), P(c + 1, r)).
 *       E(a, b, p) = (b_u - a_u) (p_v - a_v) - (b_v - a_v) (p_u - a_u).  A triangle (P0, P1, P2) is skipped when a vertex is invalid;
 *       when max(z) - min(z) > max_gap_mm; when floor(max u) - ceil(min u) >= KPX_WARP_MAX_SPAN, or the same for v (compared on the
 *       doubles, before any clamping); when area = E(P0, P1, P2) is zero or not finite.
 *   Pixels of a triangle: every integer pixel centre p = (x, y) with ceil(min u) <= x <= floor(max u), ceil(min v) <= y <= floor(max v),
 *       0 <= x <= color_width - 1, 0 <= y <= color_height - 1:   w0 = E(P1, P2, p), w1 = E(P2, P0, p), w2 = E(P0, P1, p);
 *       the pixel is inside when all three are >= 0 (area > 0) or all three are <= 0 (area < 0): an edge belongs to both triangles
 *       beside it;   s = (w0 + w1) + w2, skipped when s = 0;   zz = ((w0 z0 + w1 z1) + w2 z2) / s, zi = floor(zz + 0.5), skipped unless
 *       1 <= zi <= 65535.
 *   Warped depth of a colour pixel: the MINIMUM zi over every triangle pixel that reached it, 0 where none did -- a minimum does not
 *       depend on the order in which threads arrive.  Every output element is written.
 *   Occlusion test (kpx_color_to_depth_visible): for a depth pixel AC20 would sample, (ix, iy) = (floor(uc + 0.5), floor(vc + 0.5)) --
 *       the bilinear sampler tests this nearest pixel too: it lies inside the image when the 2 x 2 block does -- and w = warped[iy][ix];
 *       the pixel is occluded when w != 0 and q_z - (double)w > occlusion_mm, and all its channels are then zero.  Everything else is
 *       AC20's; occlusion_mm = +inf gives kpx_color_to_depth's bytes.
 * kpx_depth_to_color: depth u16 [frames][depth_height depth_width], xy f32 [calibrations][depth_height depth_width][2],
 *     out u16 [frames][color_height][color_width], all on the device, no alignment required; h_calibrations as kpx_color_to_depth.
 *     ws: kpx_depth_to_color_workspace_bytes(frames, color_width, color_height) = frames color_height color_width 4 bytes of device
 *     scratch (a 32-bit z-buffer, cleared by the call).  Asynchronous, no host read-back; frames <= 65535.  max_gap_mm >= 0, +inf allowed
 *     ("never"); NaN, negative sizes, null pointers, calibrations outside 1 .. KPX_SENSOR_MAX_CALIBRATIONS or not dividing frames,
 *     non-finite cameras or transforms and a short ws_bytes are rejected before the device is touched.  frames = 0 or an empty colour
 *     image return KPX_OK without a launch; a depth image with width < 2 or height < 2 has no triangle: out is all zeros, written.
 * kpx_color_to_depth_visible: kpx_color_to_depth with the occlusion test; warped u16 [frames][color_height][color_width] on the device,
 *     occlusion_mm >= 0 (+inf allowed). */
#define KPX_WARP_MAX_SPAN 16
size_t kpx_depth_to_color_workspace_bytes(int32_t frames, int32_t color_width, int32_t color_height);
int kpx_depth_to_color(const uint16_t *depth, const float *xy, int32_t depth_width, int32_t depth_height, int32_t frames, int32_t color_width,
                       int32_t color_height, const double *h_calibrations, int32_t calibrations, double max_gap_mm, uint16_t *out, void *ws,
                       size_t ws_bytes, void *stream);
int kpx_color_to_depth_visible(const uint16_t *depth, const float *xy, const uint8_t *color, int64_t n_px, int32_t frames, int32_t color_width,
                               int32_t color_height, int32_t channels, const double *h_calibrations, int32_t calibrations, int32_t interpolation,
                               const uint16_t *warped, double occlusion_mm, uint8_t *out, void *stream);

/* ---- lens undistortion: pinhole maps, image and depth remap (arithmetic contract AC22) ---------------------------------
 * AC20's rules hold: fp64, every multiply, add and divide rounded separately in the order written, no fused multiply-add.  The
 * undistorted camera is a distortion-free camera (fx', fy', cx', cy') with the centre and the axis of the real one: a depth value (Z
 * along the axis) does not change, there is no parallax and no occlusion, and the lens model is closed form in the direction needed
 * (target pixel -> source pixel), so an inverse remap through a stored map is exact and needs neither Newton iteration nor z-buffer.
 * kpx_undistort_map: h_camera KPX_CAMERA_DOUBLES doubles (the real lens), h_pinhole 4 doubles fx', fy', cx', cy' on the host;
 *     map f32 [out_height][out_width][2] on the device.  Per output pixel (column c, row r):
 *         x = (c - cx') / fx', y = (r - cy') / fy';   (xd, yd) = distort(x, y) of AC20;   u = fx xd + cx, v = fy yd + cy;
 *     the entry is ((float)u, (float)v), each rounded once -- or (NaN, NaN) when r2 > metric_radius metric_radius or when u or v is not
 *     finite.  One thread per pixel, one launch, no scratch, asynchronous.
 * kpx_remap_u8: src u8 [frames][src_height][src_width][channels], channels 1 or 3; map f32 [maps][out_height][out_width][2];
 *     out u8 [frames][out_height][out_width][channels]; all on the device, no alignment required.  Frame f uses map f mod maps;
 *     1 <= maps <= KPX_SENSOR_MAX_CALIBRATIONS and maps divides frames.  Output pixel (c, r) samples the frame's source image at
 *     (uc, vc) = ((double)u, (double)v) of its map entry with exactly AC20's KPX_SAMPLE_NEAREST / KPX_SAMPLE_BILINEAR rules (the same
 *     formula, the same rounding: one device function serves both).  The pixel is all zeros when the map entry has a NaN, when the
 *     nearest pixel lies outside the image, or (bilinear) when any of the four neighbours does, whatever its weight.  Every output
 *     byte is written.  One launch for the whole batch (frames <= 65535), no scratch, asynchronous.
 * kpx_remap_depth: src u16 [frames][src_height][src_width], out u16 [frames][out_height][out_width], map and frames as kpx_remap_u8.
 *         KPX_SAMPLE_NEAREST:  the source pixel (floor(uc + 0.5), floor(vc + 0.5)), copied (0 stays 0); 0 when it lies outside.
 *         KPX_SAMPLE_BILINEAR, depth aware: x0, y0, ax, ay and the four neighbours d00, d10, d01, d11 as in AC20; 0 when any neighbour
 *             lies outside the image; 0 when any of the four is 0; 0 when max - min of the four exceeds max_gap_mm (they straddle a
 *             depth edge: a blend would invent a surface between foreground and background); otherwise AC20's val, stored as
 *             floor(val + 0.5).
 *     max_gap_mm >= 0, +inf allowed ("never"); it is not read for KPX_SAMPLE_NEAREST but checked all the same.  It has no default
 *     anywhere: like AC21's it is a property of the scene and the rig.  Every output element is written.
 * Rejected before the device is touched: negative sizes, null pointers, channels, the sampling code, maps outside its range or not
 * dividing frames, a non-finite camera or pinhole target, zero focal lengths, a non-positive metric radius, a NaN or negative
 * max_gap_mm.  An empty output image or frames = 0 return KPX_OK without a launch; an empty source image gives all zeros, written. */
int kpx_undistort_map(const double *h_camera, const double *h_pinhole, int32_t out_width, int32_t out_height, float *map, void *stream);
int kpx_remap_u8(const uint8_t *src, const float *map, int32_t src_width, int32_t src_height, int32_t channels, int32_t out_width,
                 int32_t out_height, int32_t frames, int32_t maps, int32_t interpolation, uint8_t *out, void *stream);
int kpx_remap_depth(const uint16_t *src, const float *map, int32_t src_width, int32_t src_height, int32_t out_width, int32_t out_height,
                    int32_t frames, int32_t maps, int32_t interpolation, double max_gap_mm, uint16_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KINECTPX_H */
