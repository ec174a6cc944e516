/* gradslam_hip.h -- C ABI of libgradslam_hip.so: the MI355X (gfx950) hot path of gradslam's
 * point-to-plane ICP odometry and PointFusion map update.
 *
 * The reference (EdwardjkFeng/gradslam) has no FFI for this path: it is pure Python on torch ops
 * (SURVEY.md section 8b).  Each entry point below therefore replaces a *chain of torch ops* in the
 * reference, cited as file:line relative to the reference root; INTEGRATION.md shows the ctypes
 * stub a gradslam maintainer would add at that call site.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless its name starts with h_;
 *  - float tensors are fp32, row-major, densely packed; index tables are int64 rows [b,n,h,w]
 *    exactly as the reference's pc2im_bnhw; counts are int32;
 *  - images are channels-last: depth (B,L,H,W), maps (B,L,H,W,3); clouds are zero-padded
 *    (B,Nmax,C) with per-batch counts[B] (reference structures/pointclouds.py "padded" form);
 *  - 4x4 matrices are 16 contiguous floats, row-major;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *    the host, nothing allocates (capturable in a hipGraph).  Scratch comes from the caller
 *    (`ws`, sized by the matching *_ws_bytes function);
 *  - return value: 0 on success, GS_ERR_* (<0) for an invalid argument, a positive hipError_t if
 *    a launch failed.  gs_last_error() describes the last failure of the calling thread.
 */
#ifndef GRADSLAM_HIP_H
#define GRADSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 3
#define GS_OK 0
#define GS_ERR_INVALID_ARG (-1)
#define GS_ERR_WORKSPACE_TOO_SMALL (-2)
#define GS_ERR_UNSUPPORTED (-3)

typedef void *gs_stream_t;

int gs_abi_version(void);
const char *gs_last_error(void);

/* ---------------------------------------------------------------- V: depth -> vertex/normal maps
 * Replaces RGBDImages._compute_vertex_map / _compute_normal_map / _compute_global_vertex_map /
 * _compute_global_normal_map (structures/rgbdimages.py:643-762) and inverse_intrinsics
 * (geometry/projutils.py:437-450), fused into one pass.  Any output pointer may be NULL.
 * poses == NULL reproduces the "poses is None -> clone" branch (global = local). */
int gs_vertex_normal_maps(const float *depth, const float *intrinsics /* B x 16 */,
                          const float *poses /* B*L x 16 or NULL */, int B, int L, int H, int W,
                          float *vertex, float *normal, float *gvertex, float *gnormal,
                          gs_stream_t stream);

/* Adjoint of the above: given d(loss)/d(map) for any subset of the four maps (NULL = zero),
 * accumulates d/d(depth) (B,L,H,W), d/d(intrinsics) (B x 16: fx,fy,cx,cy slots) and
 * d/d(poses) (B*L x 16: R and t slots).  Outputs must be zero-initialised by the caller. */
size_t gs_vertex_normal_maps_backward_ws_bytes(int B, int L, int H, int W);
int gs_vertex_normal_maps_backward(const float *depth, const float *intrinsics, const float *poses,
                                   int B, int L, int H, int W, const float *g_vertex,
                                   const float *g_normal, const float *g_gvertex,
                                   const float *g_gnormal, float *g_depth, float *g_intrinsics,
                                   float *g_poses, void *ws, size_t ws_bytes, gs_stream_t stream);
/* Deterministic form (what backward calls under torch.use_deterministic_algorithms): the same arguments and
 * results, but the intrinsics adjoint -- shared by the L frames of a batch element (inverse_intrinsics,
 * geometry/projutils.py:437-450, used by structures/rgbdimages.py:643-762) -- is added in increasing l from a
 * workspace instead of by float atomics: the same bits from run to run.  The workspace is larger. */
size_t gs_vertex_normal_maps_backward_det_ws_bytes(int B, int L, int H, int W);
int gs_vertex_normal_maps_backward_det(const float *depth, const float *intrinsics, const float *poses,
                                       int B, int L, int H, int W, const float *g_vertex,
                                       const float *g_normal, const float *g_gvertex,
                                       const float *g_gnormal, float *g_depth, float *g_intrinsics,
                                       float *g_poses, void *ws, size_t ws_bytes, gs_stream_t stream);

/* get_alpha (slam/fusionutils.py:69-73) on an (n,3) block: clamp(exp(-|p|^2/(2 sigma^2)), eps, 1.01) */
int gs_get_alpha(const float *points, int64_t n, float sigma, float eps, float *alpha,
                 gs_stream_t stream);
int gs_get_alpha_backward(const float *points, int64_t n, float sigma, float eps,
                          const float *g_alpha, float *g_points, gs_stream_t stream);

/* ---------------------------------------------------------------- dataset front-end: raw frames -> float
 * What the reference's dataset loaders do per frame on the host (datasets/tum.py:346, :455-499; icl.py:387;
 * scannet.py:189), done on the device from the raw integer frames so that 5 instead of 16 bytes per pixel
 * cross PCIe: depth (B,Hd,Wd) = uint16 (B,Hs,Ws) / depth_scale, nearest-neighbour resize; rgb (B,Hd,Wd,3) =
 * uint8 (B,Hs,Ws,3), bilinear resize (pixel centres at +0.5), optionally / 255.  Either input may be NULL.
 * The arithmetic is float64, rounded once: depth is float32(float64(u16) / depth_scale) at source pixel
 * floor(y * (Hs / Hd)), clamped; colour is the float32 nearest the float64 bilinear value, and a same-size frame keeps
 * its values exactly (before the optional / 255).  depth_scale is taken as `float`: a scale that float32 cannot represent is rounded before the division
 * (5000, 1000 and 1 are exact).  B == 0, depth_scale <= 0 with depth given, an input whose output is NULL and two NULL
 * inputs are GS_ERR_INVALID_ARG. */
int gs_frames_from_raw(const uint16_t *depth_raw, const uint8_t *rgb_raw, int B, int Hs, int Ws, int Hd,
                       int Wd, float depth_scale, int normalise_color, float *depth, float *rgb,
                       gs_stream_t stream);

/* ---------------------------------------------------------------- generic stable compaction
 * out = rows of `src` (n_rows x row_floats fp32) whose mask byte is non-zero, order preserved;
 * *out_count = number kept.  Replaces the boolean-mask indexing x[mask] the reference uses at
 * odometry/icputils.py:654-668, slam/fusionutils.py:282,401,710-713, structures/utils.py:47-50. */
size_t gs_compact_ws_bytes(int64_t n_rows);
int gs_compact_rows(const float *src, const uint8_t *mask, int64_t n_rows, int row_floats,
                    float *out, int32_t *out_count, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Same, for up to 4 row arrays sharing one mask and one scan (h_src / h_row_floats / h_out are HOST
 * arrays of n_arrays device pointers / widths): the append of fuse_with_map compacts vertex, normal,
 * colour and alpha rows of the new pixels in one go (slam/fusionutils.py:710-713).  Rows are moved as 32-bit
 * words (any bit pattern survives); rows of h_out[a] at and beyond *out_count are not written.  n_arrays outside
 * 1..4 or a NULL member is GS_ERR_INVALID_ARG; n_rows == 0 gives *out_count = 0. */
int gs_compact_multi(int n_arrays, const float *const *h_src, const int *h_row_floats,
                     float *const *h_out, const uint8_t *mask, int64_t n_rows, int32_t *out_count,
                     void *ws, size_t ws_bytes, gs_stream_t stream);
/* Append form: the selected rows of every h_src[a] go behind the *d_count rows h_dst[a] (capacity `cap` rows)
 * already holds; *d_count advances on the device (no host round trip), d_appended / d_overflow (optional)
 * receive the number of rows appended and a flag set when rows had to be dropped for lack of capacity.
 * This is Pointclouds.append_points (structures/pointclouds.py:1203-1235) for an arena-backed map. */
size_t gs_append_rows_ws_bytes(int64_t n_rows);
int gs_append_rows(int n_arrays, const float *const *h_src, const int *h_row_floats, float *const *h_dst,
                   const uint8_t *mask, int64_t n_rows, int32_t *d_count, int cap, int32_t *d_appended,
                   int32_t *d_overflow, void *ws, size_t ws_bytes, gs_stream_t stream);
/* Adjoint of gs_compact_multi (what autograd does for x[mask] in the reference): h_out[a] (n_rows, w_a)
 * receives the compacted adjoint row of every selected row and zeros everywhere else: every one of the n_rows rows is
 * WRITTEN (the caller need not clear h_out), rejected rows with the word +0.0.  With an empty selection h_grad[a] is
 * never read, but must still be non-NULL. */
int gs_expand_multi(int n_arrays, const float *const *h_grad, const int *h_row_floats,
                    float *const *h_out, const uint8_t *mask, int64_t n_rows, void *ws, size_t ws_bytes,
                    gs_stream_t stream);

/* ---------------------------------------------------------------- D: live frame -> ICP source cloud
 * downsample_rgbdimages (odometry/icputils.py:651-669): [::ds, ::ds] sub-grid of the global
 * vertex / normal maps and the rgb image of ONE frame per batch element (L == 1), valid-depth
 * pixels only, row-major order.  Outputs are padded (B, cap, 3) with cap >= ceil(H/ds)*ceil(W/ds);
 * counts[b] receives the number of rows written for batch b.  Any of the three outputs may be NULL.
 * A pixel is valid iff depth > 0 (strict; NaN is rejected, +inf and subnormals are kept); H and W need not be multiples
 * of ds.  Rows at and beyond counts[b] are not written; an output requested without its source map, or cap below the
 * grid size, is GS_ERR_INVALID_ARG. */
size_t gs_downsample_frame_ws_bytes(int H, int W, int ds);
int gs_downsample_frame(const float *depth, const float *gvertex, const float *gnormal,
                        const float *rgb, int B, int H, int W, int ds, int cap, float *out_points,
                        float *out_normals, float *out_colors, int32_t *out_pix /* (B,cap) ds-grid pixel
                        id r*ceil(W/ds)+c of every kept row, or NULL */, int32_t *counts, void *ws,
                        size_t ws_bytes, gs_stream_t stream);

/* ---------------------------------------------------------------- P: active map points
 * find_active_map_points (slam/fusionutils.py:247-282): inverse pose, transform every map point,
 * pinhole projection, in-frame test, round-half-to-even, rows [b,n,h,w] kept in (b,n) order.
 * points: padded (B,Nmax,3); counts[B]; poses/intrinsics: B x 16.  out_rows capacity: B*Nmax rows.
 * ds > 0 additionally keeps only rows with h%ds==0 && w%ds==0 (downsample_pointclouds' filter,
 * odometry/icputils.py:596-597); ds <= 0 keeps all. */
size_t gs_project_active_ws_bytes(int B, int Nmax);
int gs_project_active(const float *points, const int32_t *counts, int B, int Nmax,
                      const float *poses, const float *intrinsics, int H, int W, int ds,
                      int64_t *out_rows, int32_t *out_count, void *ws, size_t ws_bytes,
                      gs_stream_t stream);

/* S: downsample_pointclouds' gather (odometry/icputils.py:600-619): for batch element b, gather
 * attribute rows `attr[b, n]` for every table row with row.b == b, order preserved, into a padded
 * (B, cap, C) output; counts[b] = rows written.  n_rows is read from d_n_rows (device).
 * A batch element with more than cap rows: the first cap are written, nothing beyond, and counts[b] still states
 * ALL its rows (it is not clamped to cap; consumers take min(counts[b], cap)). */
size_t gs_gather_table_rows_ws_bytes(int B);
int gs_gather_table_rows(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows,
                         const float *attr, int B, int Nmax, int C, int cap, float *out,
                         int32_t *counts, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Target cloud in pixel order: buckets the table rows (all on the ds-grid: gs_project_active with ds > 0)
 * of each batch element by their ds-grid pixel.  scan_points (B,cap,3) = map points in pixel order,
 * scan_orig (B,cap) = rank of each of them among the rows of its batch element (the index the reference's
 * downsample_pointclouds order gives it), pix_start (B, npix+1 with npix = ceil(H/ds)*ceil(W/ds)) = first
 * scan slot of every ds-grid pixel (pix_start[npix] = number of targets); tgt_pix (B,cap; optional, NULL to skip) =
 * ds-grid pixel of every row in the reference's order.  Feeds gs_icp_hints; changes no result, only the order in
 * which the exact search visits the target. */
size_t gs_bucket_by_pixel_ws_bytes(int B, int H, int W, int ds);
int gs_bucket_by_pixel(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows, int B, int H,
                       int W, int ds, const float *map_points, int Nmax, int cap, float *scan_points,
                       int32_t *scan_orig, int32_t *pix_start, int32_t *tgt_pix, void *ws, size_t ws_bytes,
                       gs_stream_t stream);

/* gs_gather_table_rows (points and normals) + gs_bucket_by_pixel fused into five launches: everything
 * gs_icp_point_to_plane needs of its target -- tgt / tgt_normals (B,cap,3) and counts (B) in the reference's
 * order, plus the search hints.  tgt_index (B,cap; optional, NULL to skip) receives the map index n of every
 * target slot (what the reverse pass scatters the target adjoints back with), tgt_pix (B,cap; optional) its
 * ds-grid pixel (gs_icp_hints.tgt_pix).
 * A batch element with more than cap rows (both entry points): slots below cap are written, nothing at or beyond cap;
 * counts[b] and pix_start still state ALL its rows (neither is clamped to cap), and scan_orig below cap may then name
 * a rank >= cap. */
size_t gs_build_icp_target_ws_bytes(int B, int H, int W, int ds);
int gs_build_icp_target(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows, int B, int H,
                        int W, int ds, const float *map_points, const float *map_normals, int Nmax,
                        int cap, float *tgt, float *tgt_normals, int32_t *counts, float *scan_points,
                        int32_t *scan_orig, int32_t *pix_start, int32_t *tgt_index, int32_t *tgt_pix,
                        void *ws, size_t ws_bytes, gs_stream_t stream);

/* keep mask of downsample_pointclouds' row filter for an arbitrary table
 * (odometry/icputils.py:596-597): mask[i] = rows[i].h % ds == 0 && rows[i].w % ds == 0 */
int gs_table_ds_mask(const int64_t *rows, int64_t n_rows, int ds, uint8_t *mask, gs_stream_t stream);

/* ---------------------------------------------------------------- K: exact 1-nearest neighbour
 * Replaces chamferdist.knn_points(src, tgt) with K=1 (call site odometry/icputils.py:200-201):
 * for each source point the squared L2 distance ((dx^2+dy^2)+dz^2, fp32, no FMA) to, and index of,
 * the nearest target point; the lowest index wins ties.  ns / nt are read from device memory
 * (d_ns, d_nt) so the call needs no host round trip; max_ns / max_nt bound the launch.
 * best: packed (dist_bits << 32 | idx) per source point, the form the J kernels consume.
 * gs_knn1 prunes target chunks by an exact fp32 AABB lower bound (same result, far fewer pairs);
 * gs_knn1_bruteforce evaluates every pair (the verifier). */
size_t gs_knn1_ws_bytes(int max_nt);
int gs_knn1(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
            const int32_t *d_nt, int max_nt, uint64_t *best, void *ws, size_t ws_bytes,
            gs_stream_t stream);
int gs_knn1_bruteforce(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                       const int32_t *d_nt, int max_nt, uint64_t *best, gs_stream_t stream);
/* unpack to the reference's output types: dist2 fp32 (ns), idx int64 (ns): the key's upper word reinterpreted and its
 * lower word zero-extended (a row without a target, key ~0, gives a NaN and 0xffffffff).  Either output may be NULL;
 * rows at and beyond *d_ns are neither read nor written. */
int gs_knn1_unpack(const uint64_t *best, const int32_t *d_ns, int max_ns, float *dist2,
                   int64_t *idx, gs_stream_t stream);

/* ---------------------------------------------------------------- J: linearise + reduce
 * gauss_newton_solve's algebra (odometry/icputils.py:203-232) fused with the normal-equation
 * products of solve_linear_system (:85-87) and the error dot product (:340): from src, tgt,
 * tgt normals and the packed nearest neighbours, accumulate
 *    H = sum a a^T (6x6), g = sum a b (6), e = sum b^2, cnt = #rows,
 * a = [n ; s x n], b = n.(d - s), over rows with dist2 < dist_thresh (dist_thresh < 0: all rows;
 * NB the reference compares the threshold with the SQUARED distance).
 * out: 44 floats = H (36, row-major) | g (6) | e | cnt (as float).  Deterministic (fixed-order
 * two-level reduction, no float atomics).
 * Contract of this entry point, gs_icp_rows and both backward forms: the threshold is the STRICT d2 < dist_thresh on the
 * squared distance the key carries (a row exactly on it is rejected; dist_thresh == 0 keeps nothing); a row whose key
 * is ~0 (no target: what gs_knn1 writes for an empty target) is invalid; rows at and beyond *d_ns (<= max_ns) are
 * neither read nor written.  max_ns == 0 is accepted: 44 zeros here, nothing written by the other three. */
size_t gs_icp_linearize_ws_bytes(int max_ns);
int gs_icp_linearize(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                     const float *tgt_normals, const uint64_t *best, float dist_thresh,
                     float *out44, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Rows form of the same algebra for API parity with gauss_newton_solve: A (ns,6), b (ns), and a
 * keep mask (ns) u8; callers compact with gs_compact_rows.  Rejected rows below *d_ns get keep = 0 and +0.0 in A and
 * b; kept rows are float32 elementwise arithmetic (each product and difference rounded on its own). */
int gs_icp_rows(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                const float *tgt_normals, const uint64_t *best, float dist_thresh, float *A,
                float *b, uint8_t *keep, gs_stream_t stream);

/* Adjoint of gs_icp_linearize: given d/dH (36), d/dg (6), d/de (1) in g_out43, accumulate
 * d/dsrc (ns,3) (plain stores) and d/dtgt, d/dnormals (nt,3) (atomic scatter-add; zero-init).
 * g_src rows below *d_ns are WRITTEN (zeros for rejected rows and rows without a target); g_tgt and g_normals are
 * ACCUMULATED into, so the caller zeroes them; targets no kept row points to are left as they were. */
int gs_icp_linearize_backward(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                              const float *tgt_normals, const uint64_t *best, float dist_thresh,
                              const float *g_out43, float *g_src, float *g_tgt, float *g_normals,
                              gs_stream_t stream);
/* Deterministic form: d/dtgt, d/dnormals (rows < *d_nt, each optional) are WRITTEN, as a pure function of the
 * inputs -- the scatter of index_select's adjoint (odometry/icputils.py:215-216; the reference's CPU
 * index_select backward is deterministic) is added up in exact fixed point and rounded once (DESIGN.md, X bar),
 * with no float atomics; d/dsrc as above. */
size_t gs_icp_linearize_backward_det_ws_bytes(int max_ns, int max_nt);
int gs_icp_linearize_backward_det(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                                  const float *tgt_normals, const int32_t *d_nt, int max_nt, const uint64_t *best,
                                  float dist_thresh, const float *g_out43, float *g_src, float *g_tgt,
                                  float *g_normals, void *ws, size_t ws_bytes, gs_stream_t stream);

/* transform_pointcloud (geometry/geometryutils.py:780-792): out = R p + t, T is a DEVICE 4x4. */
int gs_transform_points(const float *pts, const int32_t *d_n, int max_n, const float *T,
                        float *out, gs_stream_t stream);

/* ---------------------------------------------------------------- X: whole ICP loops on device
 * point_to_plane_ICP (odometry/icputils.py:310-367): LM loop with the accept/reject decision kept
 * on the device.  src (ns,3), tgt/normals (nt,3), init_T (device 4x4; NULL = identity).  Outputs: T (device 4x4),
 * optional best_last (packed NN of the last iteration's first solve) and optional trace
 * (numiters x 48 floats: H36|g6|err|new_err|damp|accept|cnt|pad).  dist_thresh < 0 == None. */
/* Optional search hints (NULL, or any member NULL, = none).  They never change a result: the
 * association stays the exact nearest neighbour with the reference's tie-break, indices are reported in
 * the reference order of `tgt`. */
typedef struct gs_icp_hints {
    const float *scan_points;   /* (nt,3) the target points in a spatially coherent scan order */
    const int32_t *scan_orig;   /* (nt) reference index (into tgt) of every scan slot; required with scan_points */
    const int32_t *src_pix;     /* (ns) ds-grid pixel id r*grid_w+c of every source point */
    const int32_t *pix_start;   /* (grid_h*grid_w+1) first scan slot of every pixel (scan order = pixel order) */
    const int32_t *tgt_pix;     /* (nt) ds-grid pixel of every target, reference order (optional; unused since ABI 3) */
    int32_t grid_w, grid_h;
    /* ABI 3: the camera the targets were bucketed with -- pose (4x4, camera -> world) and intrinsics (4x4) on the
     * device, and the grid step: a target sits in pixel (r, c) iff its projection under (cam_pose, cam_K), rounded
     * half-to-even as find_active_map_points does (slam/fusionutils.py:247-282), is the image pixel (r ds, c ds).
     * gs_build_icp_target / gs_bucket_by_pixel produce exactly that from the pose and intrinsics they are given. */
    const float *cam_pose, *cam_K;
    int32_t ds;
    /* With ALL of the above given (tgt_pix excepted) the loops associate by GRID SEARCH WITH A GEOMETRIC PROOF
     * (gs_set_grid_search): every source point examines all targets of the 3x3 grid pixels around the pixel it projects
     * to; every other target projects at least 2 ds - 0.5 image pixels away from that pixel's centre, i.e. lies outside a
     * pyramid through the camera centre, and the point's distance to the pyramid's faces bounds its distance to all of
     * them from below -- a window best strictly inside that bound IS the nearest neighbour.  Points whose proof fails
     * (no map point within centimetres) take the exact chunk-box search.  Hints never change a result (tested against
     * the brute-force scan with consistent and with scrambled hints). */
} gs_icp_hints;

/* point_to_plane_ICP (odometry/icputils.py:310-367) as one call on the device (section comment above). */
size_t gs_icp_ws_bytes(int max_ns, int max_nt);
int gs_icp_point_to_plane(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                          const float *tgt_normals, const int32_t *d_nt, int max_nt,
                          const float *init_T, int numiters, float damp, float dist_thresh,
                          const gs_icp_hints *hints, float *out_T, uint64_t *best_last,
                          float *trace, void *ws, size_t ws_bytes, gs_stream_t stream);

/* point_to_plane_gradICP (odometry/icputils.py:479-545): the smooth gradLM variant. */
int gs_icp_point_to_plane_grad(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                               const float *tgt_normals, const int32_t *d_nt, int max_nt,
                               const float *init_T, int numiters, float damp, float dist_thresh,
                               float lambda_max, float B, float B2, float nu,
                               const gs_icp_hints *hints, float *out_T, uint64_t *best_last,
                               float *trace, void *ws, size_t ws_bytes, gs_stream_t stream);

/* ---------------------------------------------------------------- X with autograd: taped loops + reverse pass
 * The differentiable form of point_to_plane_ICP / point_to_plane_gradICP (odometry/icputils.py:310-367,
 * :479-545; gradients as torch autograd derives them for the reference: through the rigid transforms,
 * the linearisation, the damped solve, se3_exp and -- gradLM only -- the damping / step gates; the
 * association indices and the LM accept/reject decisions are constants).
 * Forward: same loop and results as gs_icp_point_to_plane[_grad], but every association launch keeps its
 * cloud and neighbour array, and every step its state, in the caller's `tape` (gs_icp_tape_bytes).
 * Backward: given grad_T (device 4x4, adjoint of out_T) walks the tape in reverse on the device with no
 * host synchronisation and writes grad_src (max_ns,3), grad_tgt / grad_normals (max_nt,3, rows < *d_nt;
 * optional, NULL to skip) and grad_init_T (4x4).  grad_lm selects the gradLM variant (0: LM, parameters ignored). */
size_t gs_icp_tape_bytes(int max_ns, int numiters, int grad_lm);
int gs_icp_point_to_plane_taped(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                                const float *tgt_normals, const int32_t *d_nt, int max_nt,
                                const float *init_T, int numiters, float damp, float dist_thresh,
                                int grad_lm, float lambda_max, float B, float B2, float nu,
                                const gs_icp_hints *hints, float *out_T, uint64_t *best_last,
                                void *tape, size_t tape_bytes, void *ws, size_t ws_bytes,
                                gs_stream_t stream);
size_t gs_icp_backward_ws_bytes(int max_ns);
int gs_icp_point_to_plane_backward(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                                   const float *tgt_normals, const int32_t *d_nt, int max_nt, const float *init_T,
                                   int numiters, float dist_thresh, int grad_lm, float lambda_max,
                                   float B, float B2, float nu, const void *tape, size_t tape_bytes,
                                   const float *grad_T, float *grad_src, float *grad_tgt,
                                   float *grad_normals, float *grad_init_T, void *ws, size_t ws_bytes,
                                   gs_stream_t stream);
/* Deterministic reverse pass (torch.use_deterministic_algorithms): the same arguments and outputs; every output is a
 * pure function of the inputs, bit for bit.  The target / normal adjoints -- the scatter of index_select's adjoint,
 * odometry/icputils.py:215-216, at every iteration of :310-367 / :479-545 -- are stored per reverse launch and added
 * up afterwards in exact fixed point, rounded once (no float atomics).  The workspace grows with numiters and grad_lm. */
size_t gs_icp_backward_det_ws_bytes(int max_ns, int max_nt, int numiters, int grad_lm);
int gs_icp_point_to_plane_backward_det(const float *src, const int32_t *d_ns, int max_ns, const float *tgt,
                                       const float *tgt_normals, const int32_t *d_nt, int max_nt, const float *init_T,
                                       int numiters, float dist_thresh, int grad_lm, float lambda_max,
                                       float B, float B2, float nu, const void *tape, size_t tape_bytes,
                                       const float *grad_T, float *grad_src, float *grad_tgt,
                                       float *grad_normals, float *grad_init_T, void *ws, size_t ws_bytes,
                                       gs_stream_t stream);

/* ---------------------------------------------------------------- whole PointFusion map update
 * update_map_fusion(pointclouds, live_frame, dist_th, dot_th, sigma, inplace=True)
 * (slam/fusionutils.py:761-789 = find_correspondences :549-577 + fuse_with_map :580-722) as ONE call with no
 * host synchronisation, on a map kept in caller-owned arena arrays: map_* are (B, Nmax, C) with the rows
 * n >= map_counts[b] zero; matched points are merged in place, the unmatched valid pixels of the live frame are
 * appended behind them in (h, w) order and map_counts advances ON THE DEVICE.  Nmax is both the row stride
 * and the capacity: the caller guarantees map_counts[b] + H*W <= Nmax (stats[2] flags a violation; rows that
 * do not fit are dropped).  depth (B,H,W), rgb (B,H,W,3), intrinsics / poses (B,16; poses = the live frame's
 * pose).  stats (optional, 4 + B int32): active rows, unique correspondences, overflow flag, max normal
 * dot product (float bits), appended rows per batch element -- what the reference's warnings are raised from. */
size_t gs_pointfusion_update_ws_bytes(int B, int H, int W, int Nmax);
int gs_pointfusion_update(const float *depth, const float *rgb, const float *intrinsics, const float *poses,
                          int B, int H, int W, float *map_points, float *map_normals, float *map_colors,
                          float *map_ccounts, int32_t *map_counts, int Nmax, float dist_th, float dot_th,
                          float sigma, int32_t *stats, void *ws, size_t ws_bytes, gs_stream_t stream);

/* update_map_fusion with gradients, as ONE node per sequence (reference: torch autograd through
 * slam/fusionutils.py:654-720 and structures/pointclouds.py:1203-1235, frame after frame).
 * Forward = gs_pointfusion_update (same arguments, same in-place result) that also fills `tape`
 * (gs_pointfusion_update_tape_bytes): per pixel the map point it merged into, the ten attribute floats that point held
 * before the merge, and the row counts before the append.
 * Backward (frames in reverse order; G_* = running adjoint of the WHOLE map, (B,Nmax,C) like the map arrays, holding
 * the adjoint of the map AFTER this frame on entry and of the map BEFORE it on return): pulls G back through the merge
 * at the matched rows only (an unmatched point passes its adjoint through: x' = (c x + 0)/c), reads the appended rows'
 * adjoints out behind the previous count, writes the frame's adjoints g_vertex (local vertex map, through alpha),
 * g_gvertex, g_gnormal, g_rgb (B,H,W,3 each, fully written: a pixel whose row a clamped forward dropped, row >= Nmax,
 * receives zeros like an invalid one) and walks the arena one frame back: the MATCHED rows get the bits they held
 * before this frame and map_counts the previous counts, so that the localisation's reverse pass of the same frame
 * finds the positions and normals it ran against up to the merge's re-rounding -- an unmatched live row keeps the
 * forward's re-rounded (c x + 0) * (1 / c), map rows behind the previous count keep what the forward appended, and the
 * G_* rows behind the previous count are left as they were.  O(pixels) per frame, no host synchronisation.
 * The pair assumes that every live row has a confidence count > 0, which holds for every row these updates append
 * (alpha >= 1e-7).  On an unmatched row with count 0 in a frame that has any correspondence the forward follows the
 * reference and writes zeros (c2 == 0: inv = 1); the reference's adjoint of that row is 0 for the three attributes,
 * whereas the backward, which does not visit unmatched rows, leaves the row's G_* and its zeros in place. */
size_t gs_pointfusion_update_tape_bytes(int B, int H, int W);
int gs_pointfusion_update_taped(const float *depth, const float *rgb, const float *intrinsics, const float *poses,
                                int B, int H, int W, float *map_points, float *map_normals, float *map_colors,
                                float *map_ccounts, int32_t *map_counts, int Nmax, float dist_th, float dot_th,
                                float sigma, int32_t *stats, void *tape, size_t tape_bytes, void *ws,
                                size_t ws_bytes, gs_stream_t stream);
size_t gs_pointfusion_update_backward_ws_bytes(int B, int H, int W);
int gs_pointfusion_update_backward(const float *depth, const float *rgb, const float *intrinsics, const float *poses,
                                   int B, int H, int W, float *map_points, float *map_normals, float *map_colors,
                                   float *map_ccounts, int32_t *map_counts, int Nmax, float sigma, const void *tape,
                                   size_t tape_bytes, float *G_points, float *G_normals, float *G_colors,
                                   float *G_ccounts, float *g_vertex, float *g_gvertex, float *g_gnormal,
                                   float *g_rgb, void *ws, size_t ws_bytes, gs_stream_t stream);

/* The same for ICPSLAM's aggregate map (update_map_aggregate, slam/fusionutils.py:725-758 with inplace=True): the
 * global vertices, normals and colours of every valid live-frame pixel are appended, unmerged, in (h, w) order
 * behind the rows the arena holds; map_counts advances on the device.  stats (optional, 4 + B int32): [2] = overflow
 * flag (set in all of 0..3 when rows had to be dropped), [4 + b] = rows appended. */
size_t gs_aggregate_update_ws_bytes(int B, int H, int W);
int gs_aggregate_update(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B,
                        int H, int W, float *map_points, float *map_normals, float *map_colors,
                        int32_t *map_counts, int Nmax, int32_t *stats, void *ws, size_t ws_bytes,
                        gs_stream_t stream);

/* ---------------------------------------------------------------- differentiable localisation step
 * gs_slam_localize with autograd (the same stages; gvertex = the live frame's global vertex map under the
 * PREVIOUS pose is an input here, so that its own adjoint chains into gs_vertex_normal_maps_backward).
 * Gradients flow to gvertex (the ICP source cloud), to the map points / normals that were ICP targets, and
 * to prev_poses through the final composition -- exactly the paths torch autograd follows in the reference
 * (icpslam.py:238-247): projection / ds-grid selection / association indices are constants.
 * Backward outputs are dense and fully written: grad_gvertex (B,H,W,3), grad_map_points / grad_map_normals
 * (B,Nmax,3; optional), grad_prev_poses (B,16). */
size_t gs_slam_localize_tape_bytes(int B, int H, int W, int ds, int Nmax, int numiters, int use_grad_lm);
int gs_slam_localize_taped(const float *depth, const float *gvertex, const float *intrinsics,
                           const float *prev_poses, int B, int H, int W, int ds, const float *map_points,
                           const float *map_normals, const int32_t *map_counts, int Nmax, int use_grad_lm,
                           int numiters, float damp, float dist_thresh, float lambda_max, float Bp,
                           float B2, float nu, float *out_poses, void *tape, size_t tape_bytes, void *ws,
                           size_t ws_bytes, gs_stream_t stream);
size_t gs_slam_localize_backward_ws_bytes(int B, int H, int W, int ds, int Nmax);
int gs_slam_localize_backward(const float *prev_poses, int B, int H, int W, int ds, const float *map_points,
                              const float *map_normals, int Nmax, int use_grad_lm, int numiters,
                              float dist_thresh, float lambda_max, float Bp, float B2, float nu,
                              const void *tape, size_t tape_bytes, const float *grad_out_poses,
                              float *grad_gvertex, float *grad_map_points, float *grad_map_normals,
                              float *grad_prev_poses, int accumulate_map_grads /* 1: add into grad_map_* (a running
                              adjoint of the whole map) instead of overwriting them */,
                              void *ws, size_t ws_bytes, gs_stream_t stream);
/* Deterministic form (torch.use_deterministic_algorithms): the same arguments and outputs, bit for bit the same
 * from run to run -- each batch element's ICP reverse pass is gs_icp_point_to_plane_backward_det (the map
 * adjoints of icpslam.py:238-247 through icputils.py:215-216).  The workspace grows with numiters and use_grad_lm. */
size_t gs_slam_localize_backward_det_ws_bytes(int B, int H, int W, int ds, int Nmax, int numiters, int use_grad_lm);
int gs_slam_localize_backward_det(const float *prev_poses, int B, int H, int W, int ds, const float *map_points,
                                  const float *map_normals, int Nmax, int use_grad_lm, int numiters,
                                  float dist_thresh, float lambda_max, float Bp, float B2, float nu,
                                  const void *tape, size_t tape_bytes, const float *grad_out_poses,
                                  float *grad_gvertex, float *grad_map_points, float *grad_map_normals,
                                  float *grad_prev_poses, int accumulate_map_grads, void *ws, size_t ws_bytes,
                                  gs_stream_t stream);

/* gs_slam_localize can replay its ICP loops as a cached hipGraph once a configuration repeats (all loop
 * arguments live in the caller's workspace).  mode: 1 on, 0 off (eager launches), -1 automatic: the library
 * times its own eager launches on the host and switches to graph replay only on hosts where a launch costs
 * more than ~8 us (environment: GS_NO_GRAPH=1 / GS_GRAPH=1 force either).  Results are identical either way. */
void gs_set_graph_mode(int mode);
/* Diagnostics of that policy: out4 = {eager enqueues timed, their minimum host cost per launch in us, graphs
 * captured, graph replays}. */
int gs_graph_stats(double *out4);
/* out = T . P for B pairs of 4x4 (compose_transformations as slam/icpslam.py:245-247 uses it). */
int gs_compose_poses(const float *T, const float *P, int B, float *out, gs_stream_t stream);
/* ---------------------------------------------------------------- whole localisation step
 * ICPSLAM._localize for odom in {icp, gradicp} (slam/icpslam.py:238-247) as ONE call with no host
 * synchronisation: live-frame maps posed with the previous pose (rgbdimages.py:643-762), ds-grid
 * source cloud (icputils.py:651-669), active map points on the ds-grid of the previous frame
 * (fusionutils.py:247-282 + icputils.py:596-619), the (grad)ICP loop, and the pose composition
 * T . prev_pose (kornia compose_transformations semantics).  depth (B,H,W) is ONE frame per batch
 * element; prev_poses / out_poses are B x 16.  vertex / normal / gnormal (B,H,W,3) are optional outputs
 * (NULL to skip), gvertex is required scratch/output.  use_grad_lm selects the gradLM variant. */
size_t gs_slam_localize_ws_bytes(int B, int H, int W, int ds, int Nmax);
int gs_slam_localize(const float *depth, const float *intrinsics, const float *prev_poses, int B,
                     int H, int W, int ds, const float *map_points, const float *map_normals,
                     const int32_t *map_counts, int Nmax, int use_grad_lm, int numiters, float damp,
                     float dist_thresh, float lambda_max, float Bp, float B2, float nu,
                     float *vertex, float *normal, float *gvertex, float *gnormal, float *out_poses,
                     void *ws, size_t ws_bytes, gs_stream_t stream);

/* Optional timing of the two hot kernels of the loops above with HIP events recorded on the launch
 * stream (used by bench.py for the roofline line; off by default).  gs_profile_read folds the events
 * recorded so far (caller synchronises first) and returns launches / total ms for tag 0 = association
 * kernel, 1 = linearise kernel. */
void gs_profile_enable(int on);
int gs_profile_read(int tag, long *launches, double *total_ms);

/* How the loops above associate when ALL gs_icp_hints (camera included) are given.  1 (default; 2 is accepted as the
 * same) = grid search with its geometric proof (see gs_icp_hints), at every target density; 0 = chunk-box search always.
 * Same results bit for bit (both are the brute-force scan's); only the cost differs.  Replaces nothing in the
 * reference (chamferdist.knn_points has no such switch); for measurements and tests. */
void gs_set_grid_search(int on);

/* How gs_slam_localize and gs_slam_localize_taped build the loop's input for ONE sequence (B == 1, a ds-grid of at most
 * 24576 pixels).  1 (default) = the fused front end: three launches -- the maps' tiles with the count passes of the map's
 * projection and of the frame's ds-grid, the write pass (reference-order target, per-pixel histogram, source cloud), and the
 * target's bucketing by pixel (scan of the histogram + scatter); 0 = the separate chain (maps, count, write, pixel scan,
 * target gather / scatter).  Same results bit for bit;
 * the lines it stands for are gs_slam_localize's (slam/icpslam.py:238-247: live-frame maps, rgbdimages.py:643-762; ds-grid
 * source cloud, icputils.py:651-669; active map points on the ds-grid, fusionutils.py:247-282 + icputils.py:596-619; the
 * loop, odometry/icputils.py:310-367).  Replaces nothing in the reference; for measurements and tests. */
void gs_set_fused_setup(int on);

/* Source points per 1024-thread block of the loops' association kernel: 0 (default) = 64; 32 .. 64 = that many (tests:
 * the tile size fixes the summation order of the 6x6 system, so results of different settings agree to rounding, not bit
 * for bit; nearest neighbours are the brute-force scan's under every setting).  Replaces nothing in the reference. */
void gs_set_tile_points(int n);
/* Waves per block of the loops' association kernel: 0 (default) = automatic (eight where the grid search runs on a target of
 * at most 64 slots of capacity per grid pixel, sixteen otherwise); 8 or 16 = that many, for A/B measurements and tests.  Any other value is ignored.  Returns
 * the setting in force after the call.  Every result of the loops is the same bit for bit under either count.  The
 * environment variable GS_LOOP_WAVES (read once) does the same where the setter is at 0.  Replaces nothing in the
 * reference. */
int gs_set_loop_waves(int n);
/* Launch geometry of one association launch of the loops above for a source capacity (host-side query, no device
 * work): blocks launched, source points per block, and the number of partial rows the workspace (gs_icp_ws_bytes)
 * holds per buffer (>= blocks for every tile-size setting).  The rows are padded to at least 513: the association
 * kernel's prologue sums 512 rows unmasked (rows no block writes are kept at zero) and reads up to twelve bytes past a
 * row.  have_hints is ignored since ABI 3. */
int gs_icp_launch_geometry(int max_ns, int have_hints, int *blocks, int *tile_points_dense, int *partial_rows);
/* Counters kept on the DEVICE for the loops run so far: out4 = {loops, loops associated by grid search, loops with a
 * forced tile size (gs_set_tile_points), tiles whose point-serial straggler search overflowed its pair list and was
 * redone by the tile-level search}.  Synchronises with the device; reset != 0 zeroes the counters afterwards.  Replaces
 * nothing in the reference; lets a test assert which paths a run really exercised. */
int gs_loop_counts(unsigned int *out4, int reset);
/* Counters kept on the DEVICE for the second, re-centred window of the grid search (a lane whose first window -- centred on
 * the pixel its point projected to in the previous launch -- carried no proof looks at the 3x3 to 7x7 pixels around the pixel
 * it projects to now, before it takes the exact chunk-box search): out4 = {blocks that took the second window, lanes it
 * proved, lanes it handed on to the exact search, blocks the cap on the window's length refused (dense targets)}.
 * Synchronises with the device; reset != 0 zeroes the counters afterwards.  Replaces nothing in the reference; lets a test
 * assert which paths a run really exercised. */
int gs_window_counts(unsigned int *out4, int reset);

/* ---------------------------------------------------------------- C+U: fusion correspondences
 * find_similar_map_points (slam/fusionutils.py:381-401): keep[i] = |Vg(b,h,w) - p(b,n)| < dist_th
 * (Euclidean) && Ng(b,h,w).nrm(b,n) > dot_th for every table row; max_dot (device float, may be
 * NULL) receives the maximum dot product when that exceeds 1 and 0 otherwise (the reference warns when
 * it exceeds 1.001: un-normalised normals). */
int gs_fusion_similar(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows,
                      const float *gvertex, const float *gnormal, int H, int W,
                      const float *map_points, const float *map_normals, int Nmax, float dist_th,
                      float dot_th, uint8_t *keep, float *max_dot, gs_stream_t stream);

/* find_best_unique_correspondences (slam/fusionutils.py:489-546): per (b,h,w) keep the row
 * minimising (1/(ccount+1e-20), squared ray distance, n) compared as fp32; output rows [b,n,h,w]
 * sorted by (b,h,w).  `keep` (may be NULL = all) pre-filters rows, which fuses the compaction of
 * find_similar_map_points.  Replaces the reference's torch.unique(dim=0) row sort. */
size_t gs_fusion_unique_ws_bytes(int B, int H, int W);
int gs_fusion_unique(const int64_t *rows, const uint8_t *keep, const int32_t *d_n_rows,
                     int64_t max_rows, const float *gvertex, int B, int H, int W,
                     const float *map_points, const float *map_ccounts, int Nmax,
                     int64_t *out_rows, int32_t *out_count, void *ws, size_t ws_bytes,
                     gs_stream_t stream);

/* ---------------------------------------------------------------- F: merge matched points
 * fuse_with_map's weighted running average (slam/fusionutils.py:654-699).  EVERY map point goes
 * through the reference's formula  c' = c + alpha, x' = (c x + alpha x_f) * (1 / (c'==0 ? 1 : c'))
 * for points, normals and colours, with alpha = x_f = 0 for points that are not in `rows` (the
 * reference evaluates it on the whole padded tensors, which perturbs unmatched points by rounding;
 * that is part of its observable result).  Reads the in_* arrays (B,Nmax,C), writes the out_*
 * arrays (may alias in_* for an in-place update).  alpha (B,H,W) = get_alpha(local vertex map). */
size_t gs_fusion_merge_ws_bytes(int B, int Nmax);
int gs_fusion_merge(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows,
                    const float *gvertex, const float *gnormal, const float *rgb,
                    const float *alpha, int B, int H, int W, int Nmax, const int32_t *counts,
                    const float *in_points, const float *in_normals, const float *in_colors,
                    const float *in_ccounts, float *out_points, float *out_normals,
                    float *out_colors, float *out_ccounts, void *ws, size_t ws_bytes,
                    gs_stream_t stream);
/* Adjoint.  g_in_* (B,Nmax,C) are overwritten; g_gvertex/g_gnormal/g_rgb (B,H,W,3) and g_alpha
 * (B,H,W) receive plain stores at matched pixels only (zero-init by the caller).  Any g_* may be
 * NULL. */
int gs_fusion_merge_backward(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows,
                             const float *gvertex, const float *gnormal, const float *rgb,
                             const float *alpha, int B, int H, int W, int Nmax,
                             const int32_t *counts, const float *in_points,
                             const float *in_normals, const float *in_colors,
                             const float *in_ccounts, const float *g_out_points,
                             const float *g_out_normals, const float *g_out_colors,
                             const float *g_out_ccounts, float *g_in_points, float *g_in_normals,
                             float *g_in_colors, float *g_in_ccounts, float *g_gvertex,
                             float *g_gnormal, float *g_rgb, float *g_alpha, void *ws,
                             size_t ws_bytes, gs_stream_t stream);

/* In-place form of gs_fusion_merge for an arena-backed map: the rows that exist (n < counts[b]) are merged
 * where they are, padding is not touched, and nothing happens at all when *d_n_rows == 0 (fuse_with_map
 * skips the merge when there is no correspondence, slam/fusionutils.py:654). */
size_t gs_fusion_merge_inplace_ws_bytes(int B, int Nmax);
int gs_fusion_merge_inplace(const int64_t *rows, const int32_t *d_n_rows, int64_t max_rows,
                            const float *gvertex, const float *gnormal, const float *rgb,
                            const float *alpha, int B, int H, int W, int Nmax, const int32_t *counts,
                            float *points, float *normals, float *colors, float *ccounts, void *ws,
                            size_t ws_bytes, gs_stream_t stream);

/* ---------------------------------------------------------------- A: new-point mask
 * fuse_with_map's append mask (slam/fusionutils.py:702-707): mask = valid_depth && pixel not in
 * `rows` (B,H,W) u8.  Callers then compact gvertex/gnormal/rgb/alpha with gs_compact_rows per b. */
int gs_fusion_new_mask(const float *depth, const int64_t *rows, const int32_t *d_n_rows,
                       int64_t max_rows, int B, int H, int W, uint8_t *mask, gs_stream_t stream);

/* ---------------------------------------------------------------- R: the map rendered into a camera
 * The inverse of pointclouds_from_rgbdimages (structures/utils.py:7-57): per pixel the nearest map point that
 * find_active_map_points (slam/fusionutils.py:247-282) puts on it, as z-buffered index, depth, position, normal and colour
 * images.  The reference has no such function; a user builds it from find_active_map_points (one [b,n,h,w] row per active
 * point), a per-pixel scatter-min of the camera-frame depth over those rows, and index_select gathers of the map
 * attributes.  Here: three launches, one pass over the map with a 64-bit atomicMin per candidate, no table.
 * Candidates: rows n < min(counts[b], Nmax) that gs_project_active would keep (ds <= 0), on the pixel it reports; depth = the
 * camera-frame z (fp32).  Winner of a pixel: smallest z, ties to the smallest n; independent of arrival order.
 * Outputs (all fully written): out_index (B,H,W) int32 = winner's n or -1; out_depth (B,H,W) = its z or 0; out_points /
 * out_normals / out_colors (B,H,W,3) = its map attributes or zeros; an attribute image is skipped when its output pointer or
 * (normals, colors) its map array is NULL.  points (B,Nmax,3); poses / intrinsics: B x 16. */
size_t gs_render_map_ws_bytes(int B, int H, int W);
int gs_render_map(const float *points, const float *normals, const float *colors, const int32_t *counts,
                  int B, int Nmax, const float *poses, const float *intrinsics, int H, int W,
                  int32_t *out_index, float *out_depth, float *out_points, float *out_normals,
                  float *out_colors, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Adjoint of gs_render_map (replaces torch autograd through the gathers and the depth's rigid transform of that chain): the
 * output adjoints go to the map row each pixel shows and to the pose, with no atomics.  The pixel assignment and the winner (`index`, the forward's output) are constants.  Any of the four output adjoints may be NULL
 * (= zero); any of the four results may be NULL (= not wanted).  g_points / g_normals / g_colors (B,Nmax,3) and g_poses
 * (B x 16) are fully written: zeros for rows that won no pixel or lie beyond the count, and for the pose entries other than
 * rotation column 2 and the translation.  With z = sum_j R[j][2] (p_j - t_j):
 *   g_points[n] = g_out_points[pix] + g_depth[pix] R[:,2];  g_normals[n], g_colors[n] = their pixel's adjoint;
 *   g_poses[b][j][2] = sum_pix g_depth (p_j - t_j);  g_poses[b][j][3] = -R[j][2] sum_pix g_depth.
 * The intrinsics adjoint is zero almost everywhere and not produced.  No atomics: the same bits from run to run. */
size_t gs_render_map_backward_ws_bytes(int B, int H, int W);
int gs_render_map_backward(const float *points, const int32_t *counts, int B, int Nmax, const float *poses,
                           int H, int W, const int32_t *index, const float *g_depth,
                           const float *g_out_points, const float *g_out_normals,
                           const float *g_out_colors, float *g_points, float *g_normals, float *g_colors,
                           float *g_poses, void *ws, size_t ws_bytes, gs_stream_t stream);

/* ---------------------------------------------------------------- M: map metrics (two-sided nearest neighbours)
 * Fills the reference's empty gradslam.metrics: chamfer distance, accuracy / completeness, precision / recall / F-score and
 * Hausdorff distance all come from one call.  a (B,Na_max,3), b (B,Nb_max,3): padded fp32 clouds; a_counts / b_counts: (B,)
 * int32 on the device; rows at or beyond a count are never read.  Direction 0 searches every row of a in b, direction 1 every
 * row of b in a: the exact search of gs_knn1 (bit-identical to gs_knn1_bruteforce, the lowest index wins ties).
 *   keys_ab (B,Na_max), keys_ba (B,Nb_max): dist2_bits << 32 | index per row below the count (the others are left untouched);
 *       all ones (no neighbour) where the other cloud of the batch element is empty.
 *   stats (B,2,4) float64, per (batch element, direction) over the rows that have a neighbour, each term widened to fp64:
 *       sum d2 | sum d, d = sqrt(d2) correctly rounded in fp32 | number of rows with d2 < tau2 (strict) | max d2.
 *       Zeros when either cloud is empty.  No float atomics: the same bits from run to run.
 *   reorder != 0: each target is scanned in the order of a uniform cell grid over its bounding box (histogram, scan, scatter)
 *       so that the search prunes whatever the row order; reorder == 0: the rows are scanned as they come, as gs_knn1 does,
 *       which suits image-ordered clouds.  The results are the same bits either way.
 * Workspace, every piece rounded up to 256 bytes, with cells(N) = g^3 for the smallest g <= 64 with 16 g^2 >= N:
 *   per cloud N in (Na_max, Nb_max): 12 B N | 4 B N | 4 B N | 24 B ceil(N/16);  then 64 B | 4 B (cells(Na_max)+1) |
 *   4 B (cells(Nb_max)+1) | 32 B ceil(Na_max/64) | 32 B ceil(Nb_max/64).
 * The launch count depends neither on the counts nor on B.  Non-finite coordinates: the result is undefined (nothing is
 * written out of bounds). */
size_t gs_chamfer_ws_bytes(int B, int Na_max, int Nb_max);
int gs_chamfer(const float *a, const int32_t *a_counts, int Na_max, const float *b, const int32_t *b_counts,
               int Nb_max, int B, float tau2, int reorder, double *stats, uint64_t *keys_ab, uint64_t *keys_ba,
               void *ws, size_t ws_bytes, gs_stream_t stream);

/* Reverse pass: g2 / g1 (B,2) fp32 are the adjoints of sum d2 / sum d per direction.  For source row i with nearest row j
 * (from the keys, constants of the graph): delta = s_i - t_j, d = sqrt(d2), c = 2 g2 + (d > 0 ? g1 / d : 0); c delta goes to
 * the source's row and -c delta is scattered into the target's row j.  g_a (B,Na_max,3), g_b (B,Nb_max,3): each cloud's direct
 * part from one direction plus its scattered part from the other, written for the rows below the counts (zeros where there
 * is no neighbour); rows beyond are left untouched.  The scatter uses float atomics (arrival order) and needs no workspace
 * (ws may be NULL); the _det entry folds it in exact fixed point (four launches per batch element and direction): the same
 * bits from run to run.  Its workspace: 32 B Na_max | 32 B Nb_max | 4 | 4 max(Na_max, Nb_max) | 96 max(Na_max, Nb_max). */
size_t gs_chamfer_backward_ws_bytes(int B, int Na_max, int Nb_max);
int gs_chamfer_backward(const float *a, const int32_t *a_counts, int Na_max, const float *b,
                        const int32_t *b_counts, int Nb_max, int B, const uint64_t *keys_ab,
                        const uint64_t *keys_ba, const float *g2, const float *g1, float *g_a, float *g_b,
                        void *ws, size_t ws_bytes, gs_stream_t stream);
size_t gs_chamfer_backward_det_ws_bytes(int B, int Na_max, int Nb_max);
int gs_chamfer_backward_det(const float *a, const int32_t *a_counts, int Na_max, const float *b,
                            const int32_t *b_counts, int Nb_max, int B, const uint64_t *keys_ab,
                            const uint64_t *keys_ba, const float *g2, const float *g1, float *g_a, float *g_b,
                            void *ws, size_t ws_bytes, gs_stream_t stream);

/* ---------------------------------------------------------------- V: voxel downsampling (one row per occupied voxel)
 * The reference has no counterpart.  points (B,N_max,3): a padded fp32 batch; counts (B,) int32 on the device; voxel_size > 0
 * and origin (three floats in HOST memory, read during the call) define the grid.
 * Assignment, for batch element b and rows i < counts[b]:
 *   k = floorf((p - origin) / voxel_size) per axis: one fp32 subtraction, one IEEE fp32 division (numpy's
 *       np.floor((p - o) / v) in float32, bit for bit; floor, not truncation).  A row is valid if its three coordinates are
 *       finite and |k| < 2^20 on every axis; its key is the three biased 21-bit coordinates packed into 63 bits.
 *   Voxels are numbered 0 .. M_b - 1 in ascending order of their lowest member row (order of first appearance): a property
 *       of the input alone, not of scheduling.
 *   voxel_of (B,N_max): the voxel of every row; -1 for invalid rows (counted in n_dropped[b]) and for rows >= counts[b] (not
 *       counted).  n_voxels (B,) = M_b.  voxel_count (B,N_max): members per voxel, 0 beyond M_b.  voxel_first (B,N_max): lowest
 *       member row per voxel, -1 beyond M_b.  Every element of all five outputs is written.
 *   A hash grid per batch element: S = the smallest power of two >= 2 N_max slots, open addressing with linear probing, 64-bit
 *       compare-and-swap on the key, atomic minimum on the slot's lowest-row word; leaders (lowest member rows) are numbered by
 *       the stable compaction.  N_max <= 2^29, B <= 65535.  Every probe loop is bounded by S; should one ever run through the
 *       whole table (impossible at load <= 0.5 short of a bug) the error word is set and n_voxels is returned as -1 for every b.
 *   Five launches (six above 2^20 rows), whatever the counts and B.  Nothing synchronises the host.
 * Workspace, every piece rounded up to 256 bytes:  4 B (error word) | 8 B B S (keys) | 4 B B S (lowest rows) | 4 B B N_max
 *   (the slot of every row) | 4 B B ceil(N_max/1024) | 4 B B ceil(N_max/1024) (the compaction's block counts and offsets). */
size_t gs_voxel_assign_ws_bytes(int B, int N_max);
int gs_voxel_assign(const float *points, const int32_t *counts, int N_max, int B, float voxel_size,
                    const float *origin, int32_t *voxel_of, int32_t *n_voxels, int32_t *n_dropped,
                    int32_t *voxel_count, int32_t *voxel_first, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Reduction of a per-point attribute x (B,N_max,C) fp32, 1 <= C <= 64, over the voxels of gs_voxel_assign (voxel_of, n_voxels,
 * voxel_count as it wrote them) into out (B,M_max,C), M_max >= max_b n_voxels[b] chosen by the caller (M_max <= N_max; voxels at
 * or beyond M_max are left out).  mode: GS_VOXEL_SUM or GS_VOXEL_MEAN.  (GS_VOXEL_NO_PREAGG may be or-ed in by the timing tool:
 * the same bits without the kernel's pre-aggregation.  It is a measurement switch, NOT part of the stable contract, and may go.)
 *   sum:  out[b,m,c] = the EXACT sum of the members' values rounded once to fp32 (nearest, ties to even);
 *   mean: that fp32 value divided (IEEE fp32) by float(voxel_count[b,m]).
 *   The sum is carried in 128-bit fixed point (integer atomics), so the result does not depend on row order, arrival order or
 *   the kernel's pre-aggregation of neighbouring lanes.  Exactness domain: with lg = ceil(log2 N_max), bits more than 102 - lg
 *   binary places below the largest finite |x| among the call's members are truncated toward zero.  Non-finite members give what
 *   a float sum gives: NaN for a NaN or both infinities, else the infinity.  Rows m >= n_voxels[b] of out are written as zero:
 *   every element of out is written.  One memset and three launches.
 * Workspace, every piece rounded up to 256 bytes:  16 B B M_max C ((lo, hi) words of the sums) | 4 B B M_max ceil(C/10)
 *   (non-finite flags, 3 bits per component) | 4 B (float bits of the maximum). */
#define GS_VOXEL_SUM 0
#define GS_VOXEL_MEAN 1
#define GS_VOXEL_NO_PREAGG 2
size_t gs_voxel_reduce_ws_bytes(int B, int M_max, int C);
int gs_voxel_reduce(const float *x, const int32_t *counts, int N_max, int C, int B, const int32_t *voxel_of,
                    const int32_t *n_voxels, const int32_t *voxel_count, int M_max, int mode, float *out, void *ws,
                    size_t ws_bytes, gs_stream_t stream);

/* Reverse pass of the reduction: g_x[b,i,c] = g_out[b,m,c] (sum) or g_out[b,m,c] / float(voxel_count[b,m]) (mean) with
 * m = voxel_of[b,i]; zero where voxel_of < 0 and for rows >= counts[b]: every element of g_x (B,N_max,C) is written.  One gather
 * launch, no atomics, no workspace: the same bits from run to run.  The assignment is a constant of the graph. */
int gs_voxel_reduce_backward(const float *g_out, const int32_t *counts, int N_max, int C, int B,
                             const int32_t *voxel_of, const int32_t *voxel_count, int M_max, int mode, float *g_x,
                             gs_stream_t stream);

/* ---------------------------------------------------------------- N: neighbours (exact K nearest neighbours of every row)
 * The reference's chamferdist.knn_points takes a K and is only ever called with 1; this contract is ours.
 * src (B,Ns_max,3), tgt (B,Nt_max,3): padded fp32 clouds; src_counts / tgt_counts: (B,) int32 on the device; rows at or beyond a
 * count are never read.  1 <= K <= 32.  src == tgt (the same pointer) is the self-query: every row's first key is itself (or a
 * duplicate with a lower row).
 *   keys (B,Ns_max,K) 64-bit, EVERY element written.  For i < src_counts[b], slot k holds the k-th smallest of
 *       {(d2(i,j), j) : j < tgt_counts[b]} in lexicographic order, packed dist2_bits << 32 | j, where
 *       d2 = (dx*dx + dy*dy) + dz*dz in fp32 without FMA: the bits of gs_knn1 / gs_knn1_bruteforce, the lowest row wins ties.
 *       Slots beyond min(K, tgt_counts[b]) and all slots of rows >= src_counts[b] hold all ones (no neighbour).
 *   Search: both clouds are bucketed in one cell grid over the targets' bounding box (g cells along the longest axis, the
 *       smallest g <= 128 with kb g^2 >= tgt_counts[b], kb = K rounded up to 8 / 16 / 32); one thread per query, in the sources'
 *       cell order, keeps its sorted top K in LDS and examines a growing box of cells.  It stops only when the K-th distance is
 *       STRICTLY below a lower bound of every unexamined target (per face: the squared fp32 gap to the nearest coordinate of
 *       any target beyond it, exact by monotone rounding; no epsilon), or when nothing is left.  No result depends on g:
 *       gs_set_knn_grid(g_max) caps the cells per axis (0 = the rule) so that tests can prove it.
 *   No float atomics: the same bits from run to run, whatever the row order of either cloud.  One memset and five launches,
 *       whatever the counts, B and K.  Nothing synchronises the host.  Non-finite coordinates inside the counts: the result is
 *       undefined (nothing is written out of bounds, the search terminates).  B <= 65535.
 * Workspace, every piece rounded up to 256 bytes, with cells = g^3 for the rule's g at Nt_max:
 *   16 B B Nt_max | 4 B B Ns_max | 4 B B Ns_max | 4 B B Nt_max | 3096 B B (face tables) | 32 B B | 3072 B B (layer extremes) |
 *   4 B B cells | 4 B B cells (the two histograms).
 * Errors: GS_ERR_INVALID_ARG for a NULL pointer or a bad shape / K, GS_ERR_WORKSPACE_TOO_SMALL; a *_ws_bytes query with a bad
 * argument returns 0. */
void gs_set_knn_grid(int g_max);
size_t gs_knn_ws_bytes(int B, int Ns_max, int Nt_max, int K);
int gs_knn(const float *src, const int32_t *src_counts, int Ns_max, const float *tgt, const int32_t *tgt_counts,
           int Nt_max, int B, int K, uint64_t *keys, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Adjoint of the K distances; the keys are constants of the graph.  g_d2 (B,Ns_max,K) fp32.  A slot (i,k) is valid when its
 * key is not all ones and its row j < tgt_counts[b]; its term is v = c delta with c = 2 g_d2[i,k], delta = s_i - t_j, each
 * operation in fp32.
 *   g_src (B,Ns_max,3): ((0 + v_0) + v_1) + ... over the valid slots, k ascending, in fp32.
 *   g_tgt (B,Nt_max,3): the EXACT sum of -v over every valid slot whose neighbour is j, rounded once to fp32 (128-bit fixed
 *       point, integer atomics, as gs_voxel_reduce: with lg = ceil(log2(Ns_max K)), bits more than 102 - lg binary places below
 *       the call's largest finite |v| are truncated toward zero).  Non-finite terms give what a float sum gives.
 *   Rows beyond the counts and target rows no slot points to receive zeros: every element of both outputs is written.
 *   g_src and g_tgt must be distinct buffers, for a self-query too (the caller adds them).  One path, the same bits from run
 *   to run and under any permutation of the source rows (for g_tgt).  One memset and three launches.
 * Workspace, every piece rounded up to 256 bytes:  48 B B Nt_max | 4 B B Nt_max | 4 B. */
size_t gs_knn_backward_ws_bytes(int B, int Ns_max, int Nt_max, int K);
int gs_knn_backward(const float *src, const int32_t *src_counts, int Ns_max, const float *tgt,
                    const int32_t *tgt_counts, int Nt_max, int B, int K, const uint64_t *keys, const float *g_d2,
                    float *g_src, float *g_tgt, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Normals from the neighbourhoods, one thread per source row; not differentiable.  With x_k the target rows of the row's
 * m valid slots: m < 3 gives normal (0,0,0) and variation 0; otherwise mu = (1/m) sum x_k and C = (1/m) sum (x_k - mu)(x_k - mu)^T
 * accumulated in fp64, k ascending; the eigen-decomposition of C in fp64 by cyclic Jacobi (8 sweeps); n = the unit eigenvector of
 * the smallest eigenvalue l0, oriented, then rounded to fp32.
 *   mode 0: no orientation (the sign is whatever the decomposition gives; orient may be NULL).
 *   mode 1: orient = viewpoints (B,3); n is flipped iff n . (view_b - s_i) < 0, evaluated in fp64.
 *   mode 2: orient = reference normals (B,Ns_max,3); n is flipped iff n . ref_i < 0 (a zero reference does not flip).
 *   normals (B,Ns_max,3); variation (B,Ns_max) = l0 / (l0 + l1 + l2), 0 when the trace is 0; skipped when NULL.
 *   Rows beyond src_counts[b]: zeros.  One launch, no workspace. */
int gs_knn_normals(const float *src, const int32_t *src_counts, int Ns_max, const float *tgt,
                   const int32_t *tgt_counts, int Nt_max, int B, int K, const uint64_t *keys, int mode,
                   const float *orient, float *normals, float *variation, gs_stream_t stream);

/* ---------------------------------------------------------------- T: TSDF volumes (fuse posed RGB-D frames, extract the surface)
 * The reference has no counterpart.  A dense grid per batch element: dims (nx, ny, nz) with nx ny nz <= 2^29, edge voxel_size > 0,
 * origin (B,3) fp32 ON THE DEVICE (the corner of voxel (0,0,0)).  State, fp32, x fastest: tsdf (B,nz,ny,nx), 1 where unobserved;
 * weight (B,nz,ny,nx), 0 where unobserved; color (B,nz,ny,nx,3), optional (NULL).  B <= 65535.
 *   The centre of voxel i along axis k is  c_k = o_k + ((float)i_k + 0.5f) * voxel_size  (one rounded product, one rounded sum).
 * Integration of frames depth (B,L,H,W), rgb (B,L,H,W,3), intrinsics (B,4,4), poses (B,L,4,4); for every voxel the frames
 * l = 0 .. L-1 are applied in order:
 *   1. the centre is projected with the rule of gs_project_active (same device body): not active -> the frame is skipped;
 *   2. d = depth[b,l,h,w]; !(d > 0) -> skipped;     3. sdf = d - z (z: camera-frame depth of the centre); sdf < -trunc -> skipped;
 *   4. t = fminf(1, sdf / trunc);                   5. tsdf = (W tsdf + t) / (W + 1), every colour component the same way with
 *      rgb[b,l,h,w,k], then W = fminf(W + 1, max_weight).  IEEE fp32, no contraction.
 *   One launch per chunk of up to 32 frames (one thread per 4 consecutive x-voxels, the state in registers, the chunk's cameras in
 *   LDS; 16-byte accesses when nx is a multiple of 4 and the pointers are 16-byte aligned).  The result is what L single-frame
 *   calls give, bit for bit.  The outputs may alias the inputs.  color_in / color_out / rgb go together (all three or NULL
 *   colours).  No workspace, no atomics, nothing synchronises the host. */
int gs_tsdf_integrate(const float *depth, const float *rgb, const float *intrinsics, const float *poses, int B, int L,
                      int H, int W, int nx, int ny, int nz, float voxel_size, const float *origin, float trunc,
                      float max_weight, const float *tsdf_in, const float *weight_in, const float *color_in,
                      float *tsdf_out, float *weight_out, float *color_out, gs_stream_t stream);

/* Reverse pass of the integration.  Constants of the graph: the pixel of a voxel, the three skips, the t = 1 branch, the weight
 * cap.  Per applied frame, with W the weight before it (= weight_in, or fminf(weight_in + n, max_weight) after n >= 1 earlier updates):
 *   g_t = g / (W + 1),  g <- g (W / (W + 1)),  and g_t / trunc goes to depth[b,l,h,w] iff sdf < trunc; colours the same with rgb.
 *   g_tsdf_in (B,nz,ny,nx), g_color_in: what is left after frame 0.  g_depth (B,L,H,W), g_rgb (B,L,H,W,3): per pixel the EXACT
 *   sum of its voxels' terms rounded once to fp32 (128-bit fixed point, integer atomics, as gs_voxel_reduce: with
 *   lg = ceil(log2(nx ny nz)), bits more than 102 - lg places below the chunk's largest finite |term| are truncated toward
 *   zero; non-finite terms give what a float sum gives).  Every element of all four outputs is written; the same bits from run to
 *   run.  g_color_out / g_color_in / g_rgb go together (all three or NULL).  g_*_in may alias g_*_out.
 *   Chunks of 32 frames in reverse order, per chunk one memset and three launches; a chunk re-projects the frames before it
 *   to count its voxels' earlier updates.
 * Workspace, every piece rounded up to 256 bytes, with P = B min(L, 32) H W:  4 B (maximum) | 4 B P (flags) | 64 B P (sums). */
size_t gs_tsdf_integrate_backward_ws_bytes(int B, int L, int H, int W);
int gs_tsdf_integrate_backward(const float *depth, const float *intrinsics, const float *poses, int B, int L, int H, int W,
                               int nx, int ny, int nz, float voxel_size, const float *origin, float trunc,
                               float max_weight, const float *weight_in, const float *g_tsdf_out,
                               const float *g_color_out, float *g_tsdf_in, float *g_color_in, float *g_depth,
                               float *g_rgb, void *ws, size_t ws_bytes, gs_stream_t stream);

/* The same reverse pass with the adjoint of the poses.  The frame's update depends on the pose through z = sum_j R[j][2] (c_j - t_j)
 * alone (sdf = d - z), with the same constants of the graph; with gd = (g_t / trunc iff sdf < trunc, else 0), what depth[b,l,h,w]
 * receives from the voxel, dL/dz = -gd, and per camera, over the voxels the frame updates, S0 = sum gd, S_j = sum gd (c_j - t_j):
 *   g_poses[b,l][j][2] = -S_j,   g_poses[b,l][j][3] = R[j][2] S0,   every other entry 0 (row 3 included)
 * -- the adjoint of the unconstrained matrix entries, gs_render_map_backward's convention.  g_poses (B,L,4,4) is written in full.
 * The four other outputs are gs_tsdf_integrate_backward's, bit for bit; each may be NULL (g_color_in and g_rgb need g_color_out),
 * and what nobody asks for is not computed (without g_depth and g_rgb a chunk is two launches).  The sums are plain fp32 in one
 * fixed order, no atomics: terms gd, gd (c_j - t_j) (a rounded difference, a rounded product); per block of 256 consecutive voxels
 * the 64-lane butterfly (offsets 32, 16, .. 1), then the 4 waves in ascending order; the blocks' rows r, r + 64, .. in ascending
 * order onto +0 for r = 0 .. 63, then those 64 in ascending order.  The same bits from run to run.
 * Workspace, every piece rounded up to 256 bytes, with P = B min(L, 32) H W and N = B nx ny nz:  gs_tsdf_integrate_backward's |
 * 16 B B min(L, 32) ceil(nx ny nz / 256) (the blocks' rows) | iff L > 32: 4 B N, and with has_color 12 B N (the adjoints carried
 * from chunk to chunk when g_tsdf_in / g_color_in are NULL). */
size_t gs_tsdf_integrate_backward_poses_ws_bytes(int B, int L, int H, int W, int nx, int ny, int nz, int has_color);
int gs_tsdf_integrate_backward_poses(const float *depth, const float *intrinsics, const float *poses, int B, int L, int H,
                                     int W, int nx, int ny, int nz, float voxel_size, const float *origin, float trunc,
                                     float max_weight, const float *weight_in, const float *g_tsdf_out,
                                     const float *g_color_out, float *g_tsdf_in, float *g_color_in, float *g_depth,
                                     float *g_rgb, float *g_poses, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Surface extraction.  A voxel is observed iff weight >= min_weight.  Edge slot e = 3 j + a runs from voxel j to its +1
 * neighbour j+ along axis a (0: x, 1: y, 2: z) and exists iff that neighbour is inside the grid; it carries a point iff both
 * ends are observed and (f0 < 0) != (f1 < 0), f0 = tsdf[j], f1 = tsdf[j+].  Then s = f0 / (f0 - f1); the point is the centre of
 * j with component a moved by s voxel_size; color = col0 + s (col1 - col0); normal = g / |g| (a zero g stays zero) with
 * g = D(j) + s (D(j+) - D(j)), D_k = the difference of tsdf along axis k over the observed neighbours inside the grid
 * (central halved, else one-sided, else 0).  Rows come in ascending e per batch element (stable compaction):
 *   points, normals, colors (B,cap,3), edge (B,cap) int32: the first min(n, cap) rows are written, nothing else;
 *   n_points (B,): the full count, whatever cap.  cap = 0 (outputs may be NULL) only counts.  colors needs color.
 * Two launches for the count, one more for the rows; nothing synchronises the host.
 * Workspace, every piece rounded up to 256 bytes:  4 B B ceil(3 nx ny nz / 1024), twice (block counts and offsets). */
size_t gs_tsdf_extract_ws_bytes(int B, int nx, int ny, int nz);
int gs_tsdf_extract(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz,
                    float voxel_size, const float *origin, float min_weight, int cap, float *points, float *normals,
                    float *colors, int32_t *edge, int32_t *n_points, void *ws, size_t ws_bytes, gs_stream_t stream);

/* Reverse pass of the extraction for the rows in edge / n_points (constants): with g_s = voxel_size g_point_a +
 * sum_k g_col_k (col1_k - col0_k):  g_f0 = g_s (-f1 / (f0 - f1)^2), g_f1 = g_s (f0 / (f0 - f1)^2), g_col0 = (1 - s) g_col,
 * g_col1 = s g_col.  Normals carry no gradient.  g_tsdf (B,nz,ny,nx) and g_color (optional) are written in full: a memset, then
 * six (axis, end) passes of plain read-modify-writes (no two rows of a pass share a voxel): the same bits from run to run.
 * g_points / g_colors (B,cap,3) may be NULL (zero). */
int gs_tsdf_extract_backward(const float *tsdf, const float *color, int B, int nx, int ny, int nz, float voxel_size,
                             const int32_t *edge, const int32_t *n_points, int cap, const float *g_points,
                             const float *g_colors, float *g_tsdf, float *g_color, gs_stream_t stream);

/* Ray casting: the volume seen from the cameras intrinsics (B,4,4), poses (B,L,4,4) (camera-to-world) of height x width images,
 * on the strided grid: output pixel (i, j) of Ho = ceil(height / stride) rows and Wo = ceil(width / stride) columns is
 * full-resolution pixel (h, w) = (i stride, j stride).  IEEE fp32 in the order written, no contraction:
 *   ray     dx = ((float)w - cx) / fx, dy = ((float)h - cy) / fy, dw_i = (R_i0 dx + R_i1 dy) + R_i2,
 *           len = sqrtf((dx dx + dy dy) + 1), dz = step / len.  Sample k (1 <= k < 2^30) lies at camera depth
 *           z_k = (float)k * dz (one rounded product, never a running sum) at p_i = t_i + z_k dw_i; the ray's samples are the k
 *           with near <= z_k <= far.  Depth is z, not range.  Consecutive samples are exactly `step` apart in space.
 *   sample  per axis g = (p - o) / v - 0.5f, i = floorf(g), a = g - i; inside iff 0 <= i and i + 1 <= n - 1 on all three axes;
 *           observed iff inside and all 8 corner weights are >= min_weight.  Its value f: lerp(p, q, s) = p + s (q - p), four
 *           times along x, twice along y, once along z.  Colour the same way per component.
 *   march   in ascending k; it ends at the first observed sample with f < 0 (zero counts as outside).  The end is a hit iff
 *           sample k - 1 belongs to the ray, is observed and has f_prev >= 0; otherwise, and when no sample ends it, a miss.
 *   hit     s = f_prev / (f_prev - f), z* = ((float)(k - 1) + s) * dz, p* = t + z* dw; p* not observed -> a miss.  Colour: the
 *           interpolant at p*.  Normal: the gradient of the interpolant at p* (differences along the axis, lerped over the
 *           other two, x before y before z), divided by sqrtf((gx gx + gy gy) + gz gz); it points into free space; a zero
 *           gradient -> a miss.
 *   depth (B,L,Ho,Wo): z*, 0 on a miss; normal (B,L,Ho,Wo,3): 0 on a miss; rgb (B,L,Ho,Wo,3): 0 on a miss, goes together with
 *   color (both or neither); k_end (B,L,Ho,Wo) int32: the ending sample of a hit, 0 on a miss -- the tape of the reverse pass.
 * A thread skips the samples that the ray's clip against the box [o, o + n v] (half a voxel wider than the positions that have
 * a cell, then one sample and 2^-21 of the index wider on each side) proves to be outside; a skipped sample and an unobserved one
 * mean the same to the march, so skipping changes no result.  A ray parallel to an axis divides by nothing.  Refused before any
 * device work: stride < 1, a step that is not finite and positive, near < 0 or NaN, far NaN, L > 65535, more than 2^22 tiles of
 * 16 x 16 output pixels per image, and
 * (nx + ny + nz) voxel_size / step > 2^20 -- the bound of a thread's loop, which visits at most that many samples (+ 1040).
 * One launch, one thread per output pixel, a wave per 8x8 tile; no workspace, no atomics, nothing synchronises the host. */
int gs_tsdf_raycast(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz,
                    float voxel_size, const float *origin, const float *intrinsics, const float *poses, int L, int height,
                    int width, int stride, float step, float near, float far, float min_weight, float *depth,
                    float *normal, float *rgb, int32_t *k_end, gs_stream_t stream);

/* Reverse pass of the cast for the tape k_end (the decisions are constants of the graph; normals carry no gradient; poses,
 * intrinsics and weights receive none).  Per hit pixel the samples k - 1 and k and the hit are recomputed by the forward's
 * bodies (a tape entry whose recomputation is no hit is skipped).  With
 *   g_z = g_depth + sum_ch g_rgb_ch (grad C_ch(p*) . dw) / voxel_size
 * the 8 corners of sample k - 1 receive g_z dz (-f) / (f_prev - f)^2 times their trilinear weight (wx wy) wz, those of sample k
 * g_z dz f_prev / (f_prev - f)^2 times theirs, and the 8 corners of p* receive g_rgb times their weight into g_color.
 * g_tsdf (B,nz,ny,nx) and g_color (B,nz,ny,nx,3; goes together with color) are written in full: per voxel the EXACT sum of its
 * pixels' terms rounded once to fp32 (the fold of gs_tsdf_integrate_backward with lg = ceil(log2(2 L Ho Wo))): the same bits
 * from run to run, whatever the order.  g_depth / g_rgb may be NULL (zero).  One memset and three launches.
 * Workspace, every piece rounded up to 256 bytes, with N = B nx ny nz and C = 4 with colours, else 1:
 *   4 B (maximum) | 4 B N (flags) | 16 B N C (sums). */
size_t gs_tsdf_raycast_backward_ws_bytes(int B, int nx, int ny, int nz, int has_color);
int gs_tsdf_raycast_backward(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz,
                             float voxel_size, const float *origin, const float *intrinsics, const float *poses, int L,
                             int height, int width, int stride, float step, float min_weight, const int32_t *k_end,
                             const float *g_depth, const float *g_rgb, float *g_tsdf, float *g_color, void *ws,
                             size_t ws_bytes, gs_stream_t stream);

/* The same reverse pass with the adjoint of the poses.  Constants of the graph as above: which sample ends a ray, whether it
 * hits, the cells of p0 = p(z_{k-1}), p1 = p(z_k) and p*; dz and z_k do not depend on the pose and p = t + z R d with
 * d = (dx, dy, 1).  Per hit pixel, with a0 = g_z dz (-f) / (f_prev - f)^2, a1 = g_z dz f_prev / (f_prev - f)^2 and grad the
 * gradient of the interpolant in voxel units:
 *   u0 = a0 (grad F(p0) / v),  u1 = a1 (grad F(p1) / v),  w = sum_ch g_rgb_ch (grad C_ch(p*) / v)   (zero without colours)
 *   g_poses[b,l][i][3] = sum_pix (u0 + u1) + w,     g_poses[b,l][i][j] = sum_pix ((z_{k-1} u0 + z_k u1) + z* w)_i d_j,   row 3 zero
 * -- the adjoint of the unconstrained matrix entries.  g_poses (B,L,4,4) is written in full (zeros for a camera without hits).
 * g_tsdf and g_color are gs_tsdf_raycast_backward's, bit for bit, and may be NULL (g_color needs color and g_tsdf; without
 * g_tsdf the call is two launches).  The twelve sums are plain fp32 in one fixed order, no atomics: per block of 16 x 16 output
 * pixels the 64-lane butterfly of each 8x8 tile (offsets 32, 16, .. 1), then the 4 waves in ascending order; the blocks' rows
 * r, r + 64, .. in ascending order onto +0 for r = 0 .. 63, then those 64 in ascending order.  The same bits from run to run.
 * Workspace, every piece rounded up to 256 bytes:  gs_tsdf_raycast_backward's | 48 B B L ceil(Ho / 16) ceil(Wo / 16) (the
 * blocks' rows). */
size_t gs_tsdf_raycast_backward_poses_ws_bytes(int B, int nx, int ny, int nz, int has_color, int L, int height, int width,
                                               int stride);
int gs_tsdf_raycast_backward_poses(const float *tsdf, const float *weight, const float *color, int B, int nx, int ny, int nz,
                                   float voxel_size, const float *origin, const float *intrinsics, const float *poses, int L,
                                   int height, int width, int stride, float step, float min_weight, const int32_t *k_end,
                                   const float *g_depth, const float *g_rgb, float *g_tsdf, float *g_color, float *g_poses,
                                   void *ws, size_t ws_bytes, gs_stream_t stream);

/* Triangle meshes (marching cubes over the rows of gs_tsdf_extract).  A cube is the 8 voxels whose lowest corner is voxel j
 * (corner c = dx + 2 dy + 4 dz); it emits iff all 8 corners are observed (weight >= min_weight); its case has bit c set iff
 * tsdf < 0 at corner c (zero counts as outside, as for the edges).  The case table is generated by tools/gen_mc_table.py
 * (csrc/gs_mc_table.hpp): cube edge k = 4 a + o1 + 2 o2 runs along axis a from the corner with offsets o1, o2 on the two other
 * axes (ascending); its vertex is edge slot e = 3 j' + a of the extraction, j' the voxel at its lower end.  On an ambiguous
 * face the two segments each go round one inside corner, which the face's four signs alone decide: the two cubes sharing the
 * face agree, so the mesh is closed wherever the volume is observed.  Triangles run counter-clockwise seen from free space.
 *   edge (B,vcap) int32, n_points (B,): the rows of gs_tsdf_extract for the same volume and min_weight; a triangle's corner is
 *   the row r with edge[b,r] = e, found by binary search of edge[b, 0 .. min(n_points[b], vcap)); an e that is not there (a
 *   truncated list, vcap < n_points[b]) gives -1; nothing is read past vcap.
 *   faces (B,fcap,3) int32: ascending cube id, then table order; the first min(n, fcap) rows are written, the others hold -1;
 *   n_faces (B,): the full count, whatever fcap.  fcap = 0 (faces, edge, n_points may be NULL) only counts.
 * Refused: nx ny nz > 2^28 (5 faces per cube must fit int32).  One memset (with fcap > 0) and three launches (per-block counts,
 * per-batch-element scan, ordered write); no float atomics, nothing synchronises the host.
 * Workspace, every piece rounded up to 256 bytes:  4 B B ceil(nx ny nz / 1024), twice (block counts and offsets). */
size_t gs_tsdf_faces_ws_bytes(int B, int nx, int ny, int nz);
int gs_tsdf_faces(const float *tsdf, const float *weight, int B, int nx, int ny, int nz, float min_weight,
                  const int32_t *edge, const int32_t *n_points, int vcap, int fcap, int32_t *faces, int32_t *n_faces,
                  void *ws, size_t ws_bytes, gs_stream_t stream);

/* Dense RGB-D odometry: the transform T (B,16 row-major 4x4) that takes SOURCE-camera coordinates to TARGET-camera coordinates,
 * by Gauss-Newton on a joint photometric + depth residual over an image pyramid, coarse to fine.  Both frames per batch element
 * have depth (B,H,W), rgb (B,H,W,3) and the intrinsics (B,4,4) (fx = K[0], fy = K[5], cx = K[2], cy = K[6]; pixel centres at
 * integer coordinates).  IEEE fp32 in the order written, no contraction; u is a column, v a row.
 *   level 0    I = rgb_scale * ((0.299f R + 0.587f G) + 0.114f B);  D = depth if 0 < depth < inf, else 0 (not valid).
 *   level l+1  floor(H_l / 2) x floor(W_l / 2) pixels; pixel (u, v) reduces the block c0 = (2u, 2v), c1 = (2u+1, 2v),
 *              c2 = (2u, 2v+1), c3 = (2u+1, 2v+1) of level l:  I = (((I0 + I1) + I2) + I3) * 0.25f;  m = the smallest valid D of
 *              the block; D = s / (float)n with s the sum in the order c0..c3 (from 0) and n the number of the valid D_k with
 *              D_k - m <= depth_diff_max; 0 when n = 0.  fx, fy: * 0.5f;  cx' = (cx + 0.5f) * 0.5f - 0.5f, likewise cy.
 *   warp       source pixel (u, v) of the level with D_s = d > 0:  px = d * (((float)u - cx) / fx), py = d * (((float)v - cy) / fy),
 *              q_i = ((T_i0 px + T_i1 py) + T_i2 d) + T_i3;  q_z > 0;  iz = 1 / q_z;  x = (fx q_x) * iz + cx, y = (fy q_y) * iz + cy;
 *              i = floorf(x), j = floorf(y), 0 <= i <= W_l - 2, 0 <= j <= H_l - 2; a = x - i, b = y - j; the target's four
 *              corners c00 = (i, j), c10 = (i+1, j), c01 = (i, j+1), c11 = (i+1, j+1) all have D > 0.
 *   sample     per channel F in (I, D):  X0 = F10 - F00, X1 = F11 - F01, top = F00 + a X0, bot = F01 + a X1;
 *              F^ = top + b (bot - top);  F_x = X0 + b (X1 - X0);  F_y = bot - top  (the interpolant and its exact derivatives).
 *   residuals  r_I = I^ - I_s(u, v);  r_D = D^ - q_z;  |r_D| <= depth_diff_max.  A pixel that passes every test is valid.
 *   rows       gx = fx * iz, gy = fy * iz;  c0 = F_x gx, c1 = F_y gy, c2 = -((c0 q_x + c1 q_y) * iz), for D: ... - 1;
 *              J = w * (c0, c1, c2, q_y c2 - q_z c1, q_z c0 - q_x c2, q_x c1 - q_y c0)   (xi = [v; omega], d q / d xi = [I | -q^]),
 *              w_I = sqrtf(1 - lambda_geo), w_D = sqrtf(lambda_geo); the residuals are scaled by the same factors.
 *   sums       per valid pixel the 29 terms  J_I[m] J_I[n] + J_D[m] J_D[n] (m <= n, row-major: 21) | J_I[m] r_I + J_D[m] r_D (6) |
 *              r_I r_I + r_D r_D | 1.  Blocks of 256 consecutive pixels: six pairwise steps over a wave's 64 lanes (partners 1, 2,
 *              4 (round the 16-lane row), 8, 16 and 32 lanes away; a lane keeps half of its sums at each step and hands over
 *              the other half), the 4 waves added in order;
 *              then, per batch element, a 1024-thread block: thread (g, k) adds rows g, g + 32, ... of sum k in order, and the 32
 *              group sums are added in order.  No float atomics: the same bits from run to run.  H = the 21, g = MINUS the 6.
 *   step       cnt < 6: status bit 1, T stays.  Else xi = (H + damp I)^-1 g (damping added in fp32, the system solved in fp64),
 *              T <- exp(xi) T (the exponential and the product of the ICP step); xi or the product not finite: status bit 2,
 *              T stays.
 *   loop       from level `levels` - 1 down to 0, numiters[l] iterations at level l (a host array, finest first), from `init`
 *              (B,16; NULL: the identity).  info (B, levels, 4) floats: cnt and err of the level's last linearisation, the status
 *              bits of the level's iterations or-ed, the iterations run at the level (zeros for a level with none).
 * Two launches per iteration (linearise, one source pixel per lane; step), one per frame and level for the pyramids, one to
 * start; nothing synchronises the host, the loop state (T) lives in the workspace.  Refused before any device work: NULL
 * pointers, B outside [1, 65535], H W > 2^24, B H W > 2^30, levels outside [1, 8] or a coarsest level smaller than 4 x 4,
 * lambda_geo outside [0, 1], depth_diff_max not finite and positive, damp negative or not finite, rgb_scale not finite, a count
 * outside [0, 2^20].  Workspace, every piece rounded up to 256 bytes, with P = sum_l H_l W_l:
 *   64 B (T) | 116 B ceil(H W / 256) (partial rows) | 8 B P (target pyramid, level-major) | 8 B P (source pyramid). */
size_t gs_rgbd_odometry_ws_bytes(int B, int H, int W, int levels);
int gs_rgbd_odometry(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                     const float *intrinsics, const float *init, int levels, const int *numiters, float lambda_geo,
                     float depth_diff_max, float damp, float rgb_scale, float *out_T, float *info, void *ws, size_t ws_bytes,
                     gs_stream_t stream);
/* One level-0 linearisation at the given T (B,16): valid (B,H,W) int32, rows (B,H,W,14) = J_I | r_I | J_D | r_D (zeros where not
 * valid), sums (B,29) = H upper triangle | g | err | cnt.  The workspace of gs_rgbd_odometry_ws_bytes(B, H, W, 1). */
int gs_rgbd_rows(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                 const float *intrinsics, const float *T, float lambda_geo, float depth_diff_max, float rgb_scale, int32_t *valid,
                 float *rows, float *sums, void *ws, size_t ws_bytes, gs_stream_t stream);
/* The pyramid of one frame alone: out holds level after level, level l as (B, H_l, W_l, 2) floats (I, D). */
int gs_rgbd_pyramid(const float *depth, const float *rgb, int B, int H, int W, int levels, float depth_diff_max, float rgb_scale,
                    float *out, gs_stream_t stream);

/* The reverse pass of the dense RGB-D odometry.  It differentiates the rule above with every DECISION HELD CONSTANT: the validity
 * tests (d > 0, q_z > 0, the cell bounds, the four corner depths, |r_D| <= depth_diff_max), the cell (floor x, floor y), the
 * pyramid's foreground selection (the smallest depth m, which depths are taken, n), the depth clean-up at level 0, and whether a
 * step was applied (cnt < 6, or a solve / product that was not finite: the step is the identity and its adjoint passes through).
 * Differentiable: target depth and rgb, source depth and rgb, and rows 0..2 of `init` (the bottom row is the constant (0, 0, 0, 1):
 * its gradient is zero).  Not differentiable: the intrinsics, lambda_geo, damp, rgb_scale, info.  Only rows 0..2 of grad_T are read.
 *   tape       gs_rgbd_odometry_taped is gs_rgbd_odometry -- the same loop, the same launches, out_T and info bit for bit -- whose
 *              step also writes one row of 64 floats per (iteration, batch element), in the order the iterations run:
 *              T before the step (16) | the 29 sums as reduced (the six of g not negated) | xi (6) | 1 if the step was applied,
 *              else 0 | unused.  gs_rgbd_odometry_tape_size(B, levels, numiters) = 256 B max(numiters, 1), where numiters is
 *              the SUM of the levels' counts (in both size queries); 0 for a B, levels or sum the loop refuses.
 *   step       iterations last to first (level 0 first).  T-bar_{k+1} = the carried adjoint + the 12 sums that iteration k+1's
 *              pixel pass left (T_{k+1}'s adjoint through its linearisation).  An applied step T_{k+1} = dT T_k, dT = exp(xi),
 *              xi = (H + damp I)^-1 g:  dT-bar = T-bar_{k+1} T_k^T,  T-bar_k = dT^T T-bar_{k+1} (rows 0..2),  xi-bar from the
 *              exponential's adjoint, y = (H + damp I)^-1 xi-bar (fp64, the forward's solver),  H-bar = -y xi^T,  g-bar = y.
 *   pixels     the pixel's forward values again from the taped T_k, by the forward's operations in the forward's order; the
 *              adjoints of J_I, r_I, J_D, r_D from those of the sums; through rows, residuals and the interpolant F^, F_x, F_y to
 *              the eight corner values, to the cell coordinates (F_x's derivative in b = F_y's in a = X1 - X0: the interpolant's
 *              one second derivative inside a cell), to q, to the source pixel (I_s, d) and to T.  fp32.
 *   sums       T: 12 sums per block of 256 pixels (wave butterflies, offsets 32 .. 1, then the 4 waves in order), the blocks' rows
 *              g, g + 16, .. in order and the 16 group sums in order.  Source pixel: its own lane adds, iteration after iteration.
 *              Target corners -- many source pixels land in one cell -- : the exact fold of csrc/gs_fixed128.hpp, one per level
 *              over all its iterations, rounded once.  No float atomics: the same bits from run to run.
 *   pyramids   after all levels, coarsest to finest: a fine pixel gathers 0.25 I-bar and, where its depth was taken, D-bar / n
 *              from its coarse pixel; then level 0: rgb-bar = rgb_scale I-bar (0.299, 0.587, 0.114), depth-bar = D-bar where
 *              0 < depth < inf.
 * Three launches per iteration (step reverse; pixels; the corner terms again for the fold) and one finish per level -- two and
 * none when neither g_tgt_depth nor g_tgt_rgb is asked for: nothing else reads the corner sums; the pyramids
 * are rebuilt (the forward's workspace need not survive); nothing synchronises the host.  Outputs: g_tgt_depth (B,H,W), g_tgt_rgb
 * (B,H,W,3), g_src_depth, g_src_rgb, g_init (B,16); any may be NULL.  Workspace, every piece rounded up to 256 bytes, with
 * P = sum_l H_l W_l and N = max(sum of numiters, 1):  64 B | 128 B N (the sums' adjoints) | 48 B ceil(H W / 256) | 8 B P, twice
 * (the pyramids) | 16 B P (their adjoints) | the fold of B H W rows x 2 channels: 4 | 4 B H W | 32 B H W. */
size_t gs_rgbd_odometry_tape_size(int B, int levels, int numiters);
int gs_rgbd_odometry_taped(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H,
                           int W, const float *intrinsics, const float *init, int levels, const int *numiters, float lambda_geo,
                           float depth_diff_max, float damp, float rgb_scale, float *out_T, float *info, void *ws, size_t ws_bytes,
                           gs_stream_t stream, float *tape);
size_t gs_rgbd_odometry_bwd_ws_size(int B, int H, int W, int levels, int numiters);
int gs_rgbd_odometry_bwd(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                         const float *intrinsics, int levels, const int *numiters, float lambda_geo, float depth_diff_max, float damp,
                         float rgb_scale, const float *tape, const float *grad_T, float *g_tgt_depth, float *g_tgt_rgb, float *g_src_depth,
                         float *g_src_rgb, float *g_init, void *ws, size_t ws_bytes, gs_stream_t stream);
/* The reverse of gs_rgbd_rows: g_sums (B,29) is the adjoint of `sums` exactly as gs_rgbd_rows returns them (g is MINUS the sum);
 * err's adjoint is honoured, cnt's is ignored.  The four image gradients and g_T (B,12), rows 0..2 of T's; any may be NULL.  The
 * workspace of gs_rgbd_odometry_bwd_ws_size(B, H, W, 1, 1). */
int gs_rgbd_rows_bwd(const float *tgt_depth, const float *tgt_rgb, const float *src_depth, const float *src_rgb, int B, int H, int W,
                     const float *intrinsics, const float *T, float lambda_geo, float depth_diff_max, float rgb_scale, const float *g_sums,
                     float *g_tgt_depth, float *g_tgt_rgb, float *g_src_depth, float *g_src_rgb, float *g_T, void *ws, size_t ws_bytes,
                     gs_stream_t stream);

/* SDF odometry: a frame tracked directly against a TSDF volume (Bylow, Sturm, Kerl, Kahl, Cremers, RSS 2013), by Gauss-Newton
 * on the sum over the frame's pixels of phi(D P p)^2, phi the volume's interpolated distance: no ray cast, no association, no
 * cloud.  depth (B,H,W); intrinsics (B,4,4) (fx = K[0], fy = K[5], cx = K[2], cy = K[6]); poses P (B,16 row-major 4x4, camera
 * to world): the pose the frame carries; the volume tsdf, weight (B,nz,ny,nx), origin (B,3), voxel_size, trunc as for
 * gs_tsdf_integrate.  D (B,16) is the loop state, a WORLD-frame delta.  IEEE fp32 in the order written, no contraction.
 *   levels     level l uses the pixels (h, w) = (i s_l, j s_l) of the image, s_l = stride * 2^l: ceil(H / s_l) x ceil(W / s_l)
 *              of them, row-major.  There is no pyramid: a level only selects pixels.
 *   point      pixel (h, w) with depth d, used only if 0 < d < inf:  px = d * (((float)w - cx) / fx),
 *              py = d * (((float)h - cy) / fy),  pw_i = ((P_i0 px + P_i1 py) + P_i2 d) + P_i3,
 *              q_i = ((D_i0 pw_x + D_i1 pw_y) + D_i2 pw_z) + D_i3.
 *   sample     the cell of q by the ray cast's rule (per axis g = (q - o) / v - 0.5f, i = floorf(g), a = g - i; inside iff
 *              0 <= i and i + 1 <= n - 1; a NaN or an infinity is outside); all 8 corner weights >= min_weight; all 8 corner
 *              values f_c < 1.0f (no corner is clamped free space); f^ the trilinear interpolant (four lerps along x, two along
 *              y, one along z, lerp(p, q, s) = p + s (q - p)) and g its gradient in voxel units (differences along the axis,
 *              lerped over the other two, x before y before z).  A pixel that passes every test is valid.
 *   row        kappa = trunc / voxel_size, formed once;  r = trunc * f^;  n = kappa * g;
 *              J = (n_x, n_y, n_z, q_y n_z - q_z n_y, q_z n_x - q_x n_z, q_x n_y - q_y n_x)   (xi = [v; omega], d q / d xi = [I | -q^]).
 *   sums       per valid pixel the 29 terms  J[m] J[n] (m <= n, row-major: 21) | J[m] r (6) | r r | 1.  Blocks of 256
 *              consecutive pixels of the level's grid, in the order gs_rgbd_odometry documents: six pairwise steps over a
 *              wave's 64 lanes, the 4 waves added in order; then, per batch element, thread (g, k) of a 1024-thread block adds
 *              rows g, g + 32, ... of sum k in order, and the 32 group sums are added in order.  No float atomics: the same
 *              bits from run to run.  H = the 21, g = MINUS the 6.
 *   step       gs_rgbd_odometry's: cnt < 6: status bit 1, D stays.  Else xi = (H + damp I)^-1 g (damping added in fp32, the
 *              system solved in fp64), D <- exp(xi) D; xi or the product not finite: status bit 2, D stays.
 *   loop       from level `levels` - 1 down to 0, numiters[l] iterations at level l (a host array, finest first), from `init`
 *              (B,16; NULL: the identity).  out_T = D: the new pose is D . P (the ICP providers' convention).  info
 *              (B, levels, 4) floats as gs_rgbd_odometry's: cnt and err of the level's last linearisation, the status bits of
 *              the level's iterations or-ed, the iterations run at the level (zeros for a level with none).
 * Two launches per iteration (linearise, one pixel per lane; step) and one to start; nothing synchronises the host, the loop
 * state lives in the workspace.  Refused before any device work: NULL pointers, B outside [1, 65535], H W > 2^24,
 * B H W > 2^30, stride < 1, levels outside [1, 8] or a coarsest grid smaller than 4 x 4, dims not positive or nx ny nz > 2^29,
 * voxel_size or trunc not finite and positive, min_weight not a number, damp negative or not finite, a count outside
 * [0, 2^20].  Workspace, every piece rounded up to 256 bytes, with Hs = ceil(H / stride), Ws = ceil(W / stride):
 *   64 B (D) | 116 B ceil(Hs Ws / 256) (partial rows). */
size_t gs_sdf_odometry_ws_size(int B, int H, int W, int stride);
int gs_sdf_odometry(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *init,
                    const float *tsdf, const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc,
                    float min_weight, int stride, int levels, const int *numiters, float damp, float *out_T, float *info, void *ws,
                    size_t ws_bytes, gs_stream_t stream);
/* One level-0 linearisation at the given D (B,16): valid (B,Hs,Ws) int32, rows (B,Hs,Ws,7) = J | r (zeros where not valid),
 * sums (B,29) = H upper triangle | g | err | cnt.  The workspace of gs_sdf_odometry_ws_size(B, H, W, stride). */
int gs_sdf_rows(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *D, const float *tsdf,
                const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc, float min_weight,
                int stride, int32_t *valid, float *rows, float *sums, void *ws, size_t ws_bytes, gs_stream_t stream);

/* The reverse pass of the SDF odometry.  It differentiates the rule above with every DECISION HELD CONSTANT: the depth gate, the
 * cell a point falls in (floorf per axis and the bounds), the weight gate and the free-space gate, cnt < 6, and whether a step was
 * applied (a step that was not is the identity and its adjoint passes through).  Differentiable: depth, rows 0..2 of poses and
 * of `init` (the bottom rows are the constant (0, 0, 0, 1): their gradients are zero) and the volume's tsdf.  Not differentiable:
 * weight, origin, the intrinsics, the scalar parameters, info.  Only rows 0..2 of grad_T are read.  fp32 in the order written.
 *   tape       gs_sdf_odometry_taped is gs_sdf_odometry -- the same loop, the same launches, out_T and info bit for bit -- whose
 *              step also writes gs_rgbd_odometry_taped's row of 64 floats per (iteration, batch element), in the order the
 *              iterations run: D before the step (16) | the 29 sums as reduced | xi (6) | 1 if the step was applied, else 0.
 *   step       gs_rgbd_odometry_bwd's, iterations last to first (level 0 first): D-bar_{k+1} = the carried adjoint + the 12 sums
 *              that iteration k+1's pixel pass left; dD-bar = D-bar_{k+1} D_k^T, D-bar_k = dD^T D-bar_{k+1}, xi-bar from the
 *              exponential's adjoint, y = (H + damp I)^-1 xi-bar (fp64), H-bar = -y xi^T, g-bar = y.  The same launch adds the
 *              12 sums of the poses' adjoint that iteration k+1's pixel pass left onto the running g_poses.
 *   pixels     the pixel's forward values again at the taped D_k, by the forward's operations in the forward's order.  With M the
 *              symmetric 6 x 6 of H-bar with its diagonal doubled, gv the adjoints of the six sums J r and e2 = 2 err-bar:
 *                Jb = M J + gv r   (Jb_u = gv_u r, then + M_uk J_k for k = 0..5);   rb = e2 r, then + gv_u J_u for u = 0..5;
 *                n = J[0..2], m = Jb[3..5]:  nb = Jb[0..2] + m x q,  qb = n x m;   gb = kappa nb,  fhb = trunc rb;
 *                corner c (x + 2 y + 4 z) receives  ((fhb W_c + gb_x dW_c/da_x) + gb_y dW_c/da_y) + gb_z dW_c/da_z  with
 *                W_c = (w_x w_y) w_z, w = a at the far end of an axis and 1 - a at the near end, dW_c/da_x = (+-w_y) w_z,
 *                dW_c/da_y = (+-w_x) w_z, dW_c/da_z = +-(w_x w_y);
 *                ab = fhb g + Hess gb, Hess with a zero diagonal and H_xy = lerp((f3 - f2) - (f1 - f0), (f7 - f6) - (f5 - f4), a_z),
 *                H_xz = lerp((f5 - f4) - (f1 - f0), (f7 - f6) - (f3 - f2), a_y), H_yz = lerp((f6 - f4) - (f2 - f0), (f7 - f5) - (f3 - f1), a_x),
 *                ab_x = (fhb g_x + H_xy gb_y) + H_xz gb_z, and so on;   qb += ab / v;
 *                D-bar += qb (x) (pw, 1);   pwb_j = (D_0j qb_x + D_1j qb_y) + D_2j qb_z;   P-bar += pwb (x) (px, py, d, 1);
 *                pxb = (P_00 pwb_x + P_10 pwb_y) + P_20 pwb_z, pyb likewise with column 1,
 *                db = (((P_02 pwb_x + P_12 pwb_y) + P_22 pwb_z) + pxb ux) + pyb vy,  ux = ((float)w - cx) / fx, vy = ((float)h - cy) / fy.
 *   sums       D and P: 12 sums each per block of 256 pixels (wave butterflies, offsets 32 .. 1, then the 4 waves in order), the
 *              blocks' rows g, g + 16, .. in order and the 16 group sums in order.  depth: the pixel's own lane adds into
 *              g_depth (zeroed once), iteration after iteration, level after level.  tsdf -- many pixels land in one cell -- :
 *              ONE exact fold of csrc/gs_fixed128.hpp over B nx ny nz rows for the whole loop, at most
 *              2^ceil(log2(sum_l numiters[l] Hs_l Ws_l)) terms per voxel, rounded once.  No float atomics: the same bits from
 *              run to run.
 * Two launches per iteration (step reverse; pixels) and, when g_tsdf is asked for, the pixels of every iteration once more for
 * the fold and one finish; nothing synchronises the host.  Outputs: g_depth (B,H,W), g_poses (B,16), g_init (B,16), g_tsdf
 * (B,nz,ny,nx), each written in full; any may be NULL, and its work is skipped.
 * Memory.  These entry points own two buffers with different lifetimes, so they take them by name with a capacity (`tape`,
 * `tape_cap`; `room`, `room_cap`) instead of one (ws, ws_bytes): the tape is written by the forward pass and kept until the
 * reverse pass; the room -- 20 bytes per voxel when g_tsdf is wanted -- exists only during the reverse pass.  Both are checked
 * before any device work (code -2, "tape too small" / "room too small"); a query returns 0 for a shape the entry points refuse.
 * numiters_total is the SUM of the levels' counts, N = max(numiters_total, 1), R = ceil(Hs Ws / 256) with Hs = ceil(H / stride);
 * every piece rounded up to 256 bytes:
 *   tape   64 B (D) | 116 B R (partial rows) | 256 B N (the tape rows)
 *   room   64 B (D-bar) | 64 B (P-bar) | 128 B N (the sums' adjoints) | 48 B R (D's rows) | 48 B R (P's rows) | with want_tsdf the
 *          fold of B nx ny nz rows x 1 channel: 4 | 4 B nx ny nz | 16 B nx ny nz. */
size_t gs_sdf_odometry_tape_bytes_for(int B, int H, int W, int stride, int levels, int numiters_total);
size_t gs_sdf_odometry_bwd_room(int B, int H, int W, int stride, int levels, int numiters_total, int nx, int ny, int nz, int want_tsdf);
int gs_sdf_odometry_taped(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *init,
                          const float *tsdf, const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size,
                          float trunc, float min_weight, int stride, int levels, const int *numiters, float damp, float *out_T,
                          float *info, void *tape, size_t tape_cap, gs_stream_t stream);
int gs_sdf_odometry_bwd(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *tsdf,
                        const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc,
                        float min_weight, int stride, int levels, const int *numiters, float damp, const void *tape, size_t tape_cap,
                        const float *grad_T, float *g_depth, float *g_poses, float *g_init, float *g_tsdf, void *room, size_t room_cap,
                        gs_stream_t stream);
/* The reverse of gs_sdf_rows: g_sums (B,29) is the adjoint of `sums` exactly as gs_sdf_rows returns them (g is MINUS the sum);
 * err's adjoint is honoured, cnt's is ignored.  g_depth (B,H,W), g_poses (B,12) and g_D (B,12): rows 0..2 of P's and D's, g_tsdf
 * (B,nz,ny,nx); any may be NULL.  One level, one iteration, the same kernels.  The room of
 * gs_sdf_odometry_bwd_room(B, H, W, stride, 1, 1, nx, ny, nz, g_tsdf != NULL). */
int gs_sdf_rows_bwd(const float *depth, int B, int H, int W, const float *intrinsics, const float *poses, const float *D,
                    const float *tsdf, const float *weight, int nx, int ny, int nz, const float *origin, float voxel_size, float trunc,
                    float min_weight, int stride, const float *g_sums, float *g_depth, float *g_poses, float *g_D, float *g_tsdf,
                    void *room, size_t room_cap, gs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GRADSLAM_HIP_H */
