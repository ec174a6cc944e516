// gs_gn_step.hpp -- what the Gauss-Newton loops of the two image-aligned odometries (rgbd.hip, sdf.hip) share, stated once:
// the level and status constants, the layout of the tape row (written by rgbd_step_k<true> and sdf_step_k<true>, read by
// rgbd_step_bwd_k in gs_rgbd_bwd.hpp and sdf_step_bwd_k in gs_sdf_bwd.hpp, which rgbd.hip and sdf.hip include after this
// header), gn_init (the start-up kernels' body) and the host checks on the
// image and the loop's parameters; no kernels.  The step kernels and the lane's 29 terms stay in their units: as inlined
// functions of this header they compiled to other instructions than in place ("SDF odometry").
#pragma once

#include "gs_icp_step.hpp"  // solve6, se3_exp_dev; it brings gs_icp_reduce.hpp (reduce_partials, expand44, NACC)

namespace gs {

constexpr int GN_MAX_LEVELS = 8, GN_MIN_SIDE = 4;       // the coarsest level (grid) is at least 4 x 4
constexpr int GN_STATUS_FEW = 1, GN_STATUS_SOLVE = 2;  // fewer than 6 valid pixels | the solve (or the composed transform) was not finite
// An iteration's tape row of batch element b (GN_TAPE_WORDS floats at tape + GN_TAPE_WORDS b): T before the step (16), the 29
// sums as reduced (g not yet negated), xi (6), 1 if the step was applied else 0 -- what the reverse pass replays.
constexpr int GN_TAPE_WORDS = 64, GN_TAPE_SUMS = 16, GN_TAPE_XI = 45, GN_TAPE_APPLIED = 51;

// T[b] = out_T[b] = init[b] or the identity; info = 0.  One thread of a 256-thread block per word.
__device__ __forceinline__ void gn_init(const float *__restrict__ init, int B, int n_info, float *__restrict__ Tall,
                                        float *__restrict__ out_T, float *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 16 * B) {
        const float v = init ? init[i] : (((i & 15) % 5 == 0) ? 1.0f : 0.0f);
        Tall[i] = v;
        out_T[i] = v;
    }
    if (i < n_info) info[i] = 0.0f;
}

// ------------------------------------------------------------------ host
// The bounds on (B, H, W) both units share: 0 or the number (1..3) of the first one broken; a unit numbers its own from 4.
static inline int gn_image_fault(int B, int H, int W) {
    if (!(B >= 1 && B <= 65535)) return 1;
    if (!(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24))) return 2;
    if (!((int64_t)B * H * W <= (1 << 30))) return 3;
    return 0;
}
#define GN_REQUIRE_IMAGE(name, fault)                                                                                    \
    do {                                                                                                                 \
        GS_REQUIRE((fault) != 1, name ": B must be in [1, 65535], got %d", B);                                           \
        GS_REQUIRE((fault) != 2, name ": H x W must be positive and at most 2^24 pixels, got %d x %d", H, W);            \
        GS_REQUIRE((fault) != 3, name ": B H W must be at most 2^30, got %d x %d x %d", B, H, W);                        \
    } while (0)
#define GN_REQUIRE_LOOP(name)                                                                                                     \
    do {                                                                                                                          \
        GS_REQUIRE(damp >= 0.0f && damp < INFINITY, name ": damp must be finite and not negative, got %g", (double)damp);         \
        for (int l = 0; l < levels; ++l)                                                                                          \
            GS_REQUIRE(numiters[l] >= 0 && numiters[l] <= (1 << 20), name ": numiters[%d] must be in [0, 2^20], got %d", l, numiters[l]); \
    } while (0)

}  // namespace gs
