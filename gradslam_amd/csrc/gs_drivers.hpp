// gs_drivers.hpp -- what maps.hip, project.hip and fusion.hip define for the whole-step drivers of slam.hip.  Prototypes and
// constants only: every one of the four includes it, so each definition is checked against the declaration its caller sees.
#pragma once

#include "gs_common.hpp"
#include "gs_project.hpp"

namespace gs {

// ---- maps.hip: the maps of one frame per batch element with the riders of gs_slam_localize ((pose | intrinsics) copied to
// cam_out (B, 32)) and of gs_pointfusion_update (alpha, per-pixel correspondence state, counter block zeroed)
int vertex_normal_maps_cam(const float *depth, const float *intrinsics, const float *poses, int B, int H, int W, float *vertex,
                           float *normal, float *gvertex, float *gnormal, float *cam_out, hipStream_t st);
int vertex_normal_maps_fusion(const float *depth, const float *intrinsics, const float *poses, int B, int H, int W, float *gvertex,
                              float *gnormal, float *alpha, float sigma, float eps, unsigned long long *pix_key, unsigned int *pix_n,
                              int32_t *zero, int n_zero, hipStream_t st);

// ---- project.hip: the front end of gs_slam_localize for one sequence -- projection on the ds grid + ICP target build in 4
// launches, and the fused form in 3 (maps + counts, write, bucketing)
constexpr int kBucketPixMax = 24 * 1024;  // ds-grid pixels whose bin starts fit in LDS: the fused form's limit
size_t project_target1_ws_bytes(int H, int W, int ds, int Nmax);
int project_target1(const float *points, const int32_t *counts, int Nmax, const float *poses, const float *intrinsics, int H, int W, int ds,
                    const float *map_normals, int cap, int64_t *rows, int32_t *nrows, float *tgt, float *tnrm, int32_t *nt,
                    float *scan_points, int32_t *scan_orig, int32_t *pix_start, int32_t *tgt_index, int32_t *tgt_pix, void *ws,
                    size_t ws_bytes, hipStream_t st, const DsJob *frame);
int project_front1(const float *depth, const float *points, const int32_t *counts, int Nmax, const float *poses, const float *intrinsics,
                   int H, int W, int ds, const float *map_normals, int cap, float *vertex, float *normal, float *gvertex, float *gnormal,
                   float *cam_out, int32_t *row_pix, float *tgt, float *tnrm, int32_t *nt, int32_t *tgt_index, float *scan_points,
                   int32_t *scan_orig, int32_t *pix_start, const DsJob &frame, void *ws, size_t ws_bytes, hipStream_t st);

// ---- fusion.hip: the PointFusion update's correspondence chain, merge, append and last launch; its tape and reverse pass;
// gs_aggregate_update's append of every valid pixel
size_t fusion_corr_state_bytes(int B, int H, int W, int Nmax);
void fusion_corr_init_ptrs(void *state, int B, int H, int W, int Nmax, unsigned long long **pix_key, unsigned int **pix_n);
int fusion_correspond(void *state, const float *map_points, const float *map_normals, const float *map_ccounts, const int32_t *counts,
                      int B, int Nmax, const float *poses, const float *intrinsics, int H, int W, const float *gvertex,
                      const float *gnormal, float dist_th, float dot_th, int32_t *ctr, hipStream_t st);
int fusion_merge_corr(void *state, const int32_t *ctr, const float *gvertex, const float *gnormal, const float *rgb, const float *alpha,
                      int B, int H, int W, int Nmax, const int32_t *counts, float *points, float *normals, float *colors, float *ccounts,
                      hipStream_t st);
int fusion_append_corr(void *state, int B, int H, int W, int Nmax, int b, const float *depth, const float *const *h_src,
                       const int *h_row_floats, float *const *h_dst, const int32_t *d_count, int cap, int *d_total, void *cws,
                       hipStream_t st);
int fusion_finish(void *state, int B, int H, int W, int Nmax, int32_t *ctr, int32_t *counts, const int *totals, int cap, int32_t *appended,
                  int32_t *stats, hipStream_t st);
size_t append_scratch_bytes(int64_t HW);  // the `cws` of the append passes below: one frame's compaction scratch with its total
size_t fusion_tape_bytes(int B, int H, int W);
int fusion_tape_record(const void *state, void *tape, int B, int H, int W, int Nmax, const int32_t *counts, const float *points,
                       const float *normals, const float *colors, const float *ccounts, hipStream_t st);
int fusion_tape_appended(void *tape, int B, int H, int W, const int32_t *appended, hipStream_t st);
int fusion_update_reverse(const void *tape, int B, int H, int W, int Nmax, const float *depth, const float *gvertex, const float *gnormal,
                          const float *rgb, const float *alpha, float *points, float *normals, float *colors, float *ccounts,
                          int32_t *counts, float *Gp, float *Gn, float *Gc, float *Gcc, float *g_gvertex, float *g_gnormal, float *g_rgb,
                          float *g_alpha, void *cws, hipStream_t st);
int append_valid_pixels(int n_arrays, const float *depth_b, int64_t HW, const float *const *h_src, const int *h_row_floats,
                        float *const *h_dst, int32_t *d_count, int cap, int32_t *d_appended, int32_t *d_overflow, void *cws,
                        hipStream_t st);

}  // namespace gs
