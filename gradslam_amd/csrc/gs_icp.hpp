// gs_icp.hpp -- what icp.hip defines for the other translation units (slam.hip).
#pragma once

#include "gs_common.hpp"

namespace gs {

bool profiling_enabled();  // gs_profile_enable(1) is in force
// gs_icp_point_to_plane[_grad|_taped] with the pose composition folded into the loop's last launch
// (compose_out = out_T . compose_right; both optional)
int icp_localize_run(int grad_lm, const float *src, const int32_t *d_ns, int max_ns, const float *tgt, const float *nrm,
                     const int32_t *d_nt, int max_nt, int numiters, float damp, float thresh, float lambda_max, float Bp,
                     float B2, float nu, const gs_icp_hints *hints, float *out_T, void *ws, size_t ws_bytes, hipStream_t st,
                     void *tape, size_t tape_bytes, const float *compose_right, float *compose_out);
int icp_config_stamp();  // the process-wide search / tiling switches, as one number

}  // namespace gs
