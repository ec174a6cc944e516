// gs_icp_step.hpp -- the O(1) step (X) of an ICP iteration: loop state, 6x6 solve, SE(3) exponential, LM / gradLM
// control, the step by one wave (step_wave0).  Device functions and types only, no kernel: any translation unit may include it
// (icp.hip, whose icp_step_k is the step as a launch of its own; rgbd.hip and gs_se3_bwd.hpp for solve6 and se3_exp_dev).
//
// X  the O(1) step of an iteration (reduce the partials, LM / gradLM decision, fp64 6x6 solve, SE(3)
//    exponential) runs in the prologue of the NEXT association launch: every block recomputes it on its wave 0
//    (no block barriers inside; the other waves stage the grid search meanwhile), block 0 publishes it; only a loop's
//    last step is a launch of its own.  Buffers are addressed through device-side role indices, so accept/reject
//    needs no host round trip and no copies.  What is constant over a loop (pointers, hints, parameters) is read from
//    a LoopConst in the workspace, not from kernel arguments: the SGPR count decides whether two blocks share a CU.
#pragma once

#include "gs_icp_reduce.hpp"

namespace gs {

// Device-resident loop state.  Point clouds ping-pong between pts[0..1] and nearest-neighbour arrays
// between best[0..1]; `p_cur` / `b_cur` say which one holds the current cloud.
struct IcpState {
    float T[16];    // accumulated transform
    float dT[16];   // step the next association launch applies
    float cur[44];  // H|g|e|cnt of the current cloud
    float xi[6];
    float damp;
    int p_cur;      // pts[p_cur] = current cloud; the association writes pts[1 - p_cur]
    int b_cur;      // best[b_cur] = NN of the current cloud; the association writes best[1 - b_cur]
    int b_first;    // NN buffer of the cloud the last iteration's first solve used
    int it;
};

// Clouds and nearest-neighbour arrays live in numbered slots.  The plain loops use two of each and
// ping-pong; the taped loops (autograd) give every association launch a slot of its own, so the tape
// IS the loop's working storage and nothing is copied.
struct LoopBufs {
    float *pts;                  // slot s at pts + s * pts_stride (floats)
    unsigned long long *best;    // slot s at best + s * best_stride
    int64_t pts_stride, best_stride;
    __host__ __device__ float *P(int s) const { return pts + s * pts_stride; }
    __host__ __device__ unsigned long long *N(int s) const { return best + s * best_stride; }
};

// ------------------------------------------------------------------ X: O(1) algebra on one lane
// x = (H + damp I)^-1 g.  H, g arrive in fp32 and the damping is added in fp32 like the reference
// (odometry/icputils.py:86-87); the 6x6 system itself is solved in fp64 with partial pivoting, which
// removes the solver's own rounding from the parity budget (the reference inverts in fp32 LAPACK).
// The augmented matrix lives in caller-provided memory (LDS in the kernels: dynamic indexing there costs neither
// registers nor scratch -- this rare path must not inflate the register budget of the association kernel).
__device__ __noinline__ void solve6_lu(const float *H, const float *g, float damp, float *x, double *Mbuf /* 42 */) {
    double (*M)[7] = reinterpret_cast<double (*)[7]>(Mbuf);
    // every loop stays a loop (#pragma nounroll): this is the rare path, it must stay small in registers
#pragma nounroll
    for (int i = 0; i < 6; ++i) {
#pragma nounroll
        for (int j = 0; j < 6; ++j) M[i][j] = (double)(i == j ? H[6 * i + j] + damp : H[6 * i + j]);
        M[i][6] = (double)g[i];
    }
#pragma nounroll
    for (int c = 0; c < 6; ++c) {
        int p = c;
        double big = fabs(M[c][c]);
#pragma nounroll
        for (int r = c + 1; r < 6; ++r)
            if (fabs(M[r][c]) > big) { big = fabs(M[r][c]); p = r; }
        if (p != c) {
#pragma nounroll
            for (int k = 0; k < 7; ++k) { const double t = M[c][k]; M[c][k] = M[p][k]; M[p][k] = t; }
        }
        const double piv = M[c][c];
#pragma nounroll
        for (int r = c + 1; r < 6; ++r) {
            const double f = M[r][c] / piv;
#pragma nounroll
            for (int k = c; k < 7; ++k) M[r][k] -= f * M[c][k];
        }
    }
#pragma nounroll
    for (int r = 5; r >= 0; --r) {  // the solution overwrites the right-hand side column
        double v = M[r][6];
#pragma nounroll
        for (int k = r + 1; k < 6; ++k) v -= M[r][k] * M[k][6];
        M[r][6] = v / M[r][r];
    }
#pragma nounroll
    for (int i = 0; i < 6; ++i) x[i] = (float)M[i][6];
}

// H + damp I is symmetric positive definite in every sane case (H = A^T A, damp > 0): fully unrolled
// fp64 LDL^T in registers (~0.5 us on one lane); anything else falls back to the pivoted elimination.
__device__ void solve6(const float *H, const float *g, float damp, float *x, double *lu_buf) {
    double A[6][6], d[6], y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) A[i][j] = (double)(i == j ? H[6 * i + j] + damp : H[6 * i + j]);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < j) dj -= A[j][k] * A[j][k] * d[k];
        d[j] = dj;
        ok = ok && (dj > 0.0) && (dj < 1e300);
        const double inv = 1.0 / dj;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i > j) {
                double v = A[i][j];
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k < j) v -= A[i][k] * A[j][k] * d[k];
                A[i][j] = v * inv;  // L[i][j]
            }
        }
    }
    if (!ok) {
        solve6_lu(H, g, damp, x, lu_buf);
        return;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {  // L y = g
        double v = (double)g[i];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < i) v -= A[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {  // L^T x = D^-1 y
        double v = y[i] / d[i];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k > i) v -= A[k][i] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = (float)y[i];
}

// reference geometry/se3utils.py:77-115 (xi = [v ; omega]); small-angle branch uses V = I + w^ (sic)
__device__ __noinline__ void se3_exp_dev(const float *xi, float *T) {
    const float v0 = xi[0], v1 = xi[1], v2 = xi[2], w0 = xi[3], w1 = xi[4], w2 = xi[5];
    float Wh[9] = {0.0f, -w2, w1, w2, 0.0f, -w0, -w1, w0, 0.0f};
    const float th = sqrtf(__fmaf_rn(w2, w2, __fmaf_rn(w1, w1, w0 * w0)));
    float R[9], V[9];
    if (th < 1e-6f) {
        for (int i = 0; i < 9; ++i) { R[i] = ((i % 4 == 0) ? 1.0f : 0.0f) + Wh[i]; V[i] = R[i]; }
    } else {
        const float s = sinf(th), c = cosf(th);
        float W2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                W2[3 * i + j] = dot3_fma(Wh[3 * i], Wh[3 * i + 1], Wh[3 * i + 2], Wh[j], Wh[3 + j], Wh[6 + j]);
        const float A = s / th, Bc = (1.0f - c) / (th * th), C = (th - s) / (th * th * th);
        for (int i = 0; i < 9; ++i) {
            const float e = (i % 4 == 0) ? 1.0f : 0.0f;
            R[i] = (e + A * Wh[i]) + Bc * W2[i];
            V[i] = (e + Bc * Wh[i]) + C * W2[i];
        }
    }
    for (int i = 0; i < 3; ++i) {
        T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2];
        T[4 * i + 3] = dot3_fma(V[3 * i], V[3 * i + 1], V[3 * i + 2], v0, v1, v2);
    }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

enum StepMode { STEP_ADOPT = 0, STEP_LM = 1, STEP_GRAD_B = 2 };

// Tape record of one step (REC_WORDS floats): the IcpState BEFORE the step, then what the step saw.
// The state after step j is the state before step j+1, so record j+1's head doubles as "after j".
constexpr int REC_STATE = 0;     // sizeof(IcpState)/4 words
constexpr int REC_LIN = 96;      // 44 floats: H|g|e|cnt of the cloud the preceding association wrote
constexpr int REC_SLOT = 140;    // slot that association wrote
constexpr int REC_MODE = 141;
constexpr int REC_ACCEPT = 142;
constexpr int REC_WORDS = 160;

struct GradParams {
    // formed in double on the host like the reference's Python scalars, rounded once:
    // lambda_min = 1/lambda_max, range = lambda_max - lambda_min, inv_nu = 1/nu
    float lambda_min, range, B, B2, inv_nu;
};


// x = (H + damp I)^-1 g by ONE WAVE: Gauss-Jordan on the augmented 6x7 system in fp64, element (i, k) in
// lane 8 i + k, rows / columns exchanged with lane permutes.  Takes ~0.5 us like a fully unrolled
// single-lane factorisation but needs a handful of VGPRs instead of ~100, which is what lets the step live in
// the association kernel without costing it its occupancy.  H + damp I is symmetric positive definite in
// every sane case (H = A^T A, damp > 0): no pivoting; a pivot that is not a positive finite number hands the
// system to the pivoted elimination below (one lane, matrix in LDS).  All 64 lanes must call this.
__device__ __forceinline__ double shfl_d(double v, int src) {
    const int lo = __shfl(__double2loint(v), src, kWave), hi = __shfl(__double2hiint(v), src, kWave);
    return __hiloint2double(hi, lo);
}
// (the elimination itself: `a` = the lane's element of the augmented system, element (i, k) in lane 8 i + k; returns the
// lane's element of the result -- column 6 is the solution -- and whether every pivot was a positive finite number)
__device__ __forceinline__ double solve6_wave_elim(double a, bool &ok) {
    const int lane = threadIdx.x & 63, i = lane >> 3, k = lane & 7;
    ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double piv = shfl_d(a, 8 * j + j);
        ok = ok && (piv > 0.0) && (piv < 1e300);
        const double pr = shfl_d(a, 8 * j + k);                 // pivot row, my column
        const double col = shfl_d(a, 8 * (i < 6 ? i : 0) + j);  // my row, pivot column
        const double inv = 1.0 / piv;
        a = (i == j) ? pr * inv : a - (col * inv) * pr;
    }
    return a;
}
__device__ void solve6_wave(const float *H, const float *g, float damp, float *x, double *lu_buf) {
    const int lane = threadIdx.x & 63, i = lane >> 3, k = lane & 7;
    double a = 0.0;
    if (i < 6 && k < 6) a = (double)(i == k ? H[6 * i + k] + damp : H[6 * i + k]);
    if (i < 6 && k == 6) a = (double)g[i];
    bool ok;
    a = solve6_wave_elim(a, ok);
    if (i < 6 && k == 6) x[i] = (float)a;
    if (!ok && lane == 0) solve6_lu(H, g, damp, x, lu_buf);     // `ok` is wave-uniform: every lane saw the same pivots
}

// se3_exp_dev by one wave: the lane's element (threadIdx.x & 15, row-major) of the 4 x 4 transform.  Lane m < 9 forms
// element m of R and of V, the translation's lanes fetch their row of V with lane permutes; sin / cos / A / Bc / C are
// computed once (by every lane, on the same operands).  Every element is the result of exactly se3_exp_dev's operations in
// se3_exp_dev's order: same bits.  All 64 lanes must call this.
__device__ __forceinline__ float se3_exp_wave(const float (&xi)[6]) {
    const int lane = threadIdx.x & 63;
    const float v0 = xi[0], v1 = xi[1], v2 = xi[2], w0 = xi[3], w1 = xi[4], w2 = xi[5];
    // Wh = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0}
    auto wh = [&](int q) {
        float r = 0.0f;
        r = q == 1 ? -w2 : r; r = q == 2 ? w1 : r; r = q == 3 ? w2 : r;
        r = q == 5 ? -w0 : r; r = q == 6 ? -w1 : r; r = q == 7 ? w0 : r;
        return r;
    };
    const float th = sqrtf(__fmaf_rn(w2, w2, __fmaf_rn(w1, w1, w0 * w0)));
    const int m = min(lane, 8), mi = m / 3, mj = m - 3 * mi;
    const float e = (m % 4 == 0) ? 1.0f : 0.0f, whm = wh(m);
    float Rm, Vm;
    if (th < 1e-6f) {  // (wave-uniform)
        Rm = e + whm; Vm = Rm;
    } else {
        const float s = sinf(th), c = cosf(th);
        const float W2m = dot3_fma(wh(3 * mi), wh(3 * mi + 1), wh(3 * mi + 2), wh(mj), wh(3 + mj), wh(6 + mj));
        const float A = s / th, Bc = (1.0f - c) / (th * th), C = (th - s) / (th * th * th);
        Rm = (e + A * whm) + Bc * W2m;
        Vm = (e + Bc * whm) + C * W2m;
    }
    const int t = lane & 15, i = min(t >> 2, 2), j = t & 3;
    const float r = __shfl(Rm, 3 * i + min(j, 2), kWave);
    const float va = __shfl(Vm, 3 * i, kWave), vb = __shfl(Vm, 3 * i + 1, kWave), vc = __shfl(Vm, 3 * i + 2, kWave);
    const float tr = dot3_fma(va, vb, vc, v0, v1, v2);
    if (t >= 12) return t == 15 ? 1.0f : 0.0f;
    return j == 3 ? tr : r;
}

// The O(1) step by ONE wave (S and acc in LDS).  The work is spread
// over its lanes where the data is wide -- expanding the 29 sums to H | g | e | n, adopting them, T = dT . T, the
// tape / trace records -- so that the serial part is a handful of scalars:
//   STEP_ADOPT : the look-ahead cloud becomes the current one unconditionally (initial cloud; gradICP's
//                re-linearisation)                          -> solve ; dT = exp(xi)
//   STEP_LM    : look-ahead cloud: accept (adopt, damp/2, T = dT T) or reject (damp*2) -> solve ; dT
//   STEP_GRAD_B: look-ahead error -> damp, sigma ; dT = exp(sigma xi) ; T = dT T ; look-ahead discarded
// `solve` = false for a loop's very last step, whose xi / dT nothing consumes.
// ORDER.  The chain that the block waits for is  sums -> decision -> solve -> exp.  So the solve takes its operands
// straight from the sums and the old state (lane (i, k): its element of either, selected on the decision; the new damping
// formed in a register), one LDS trip after the sums are there, and the exponential takes xi from the solve's registers.
// The bookkeeping -- adopting the 44 values, T = dT . T, the state words, the tape / trace records -- consists of stores
// whose values are in registers by then; nothing on the chain reads them back.  Same operands, same operations: same bits.
__device__ __forceinline__ float expand_elem(const float *acc, int t) {  // element t of the 44 from the 29 sums
    if (t < 36) {
        int u = t / 6, v = t % 6;
        if (u > v) { const int w = u; u = v; v = w; }
        return acc[u * 6 - (u * (u - 1)) / 2 + (v - u)];
    }
    if (t < 42) return acc[21 + (t - 36)];
    return t == 42 ? acc[27] : acc[28];
}
// LDS hand-offs inside ONE wave: its LDS operations execute in issue order, so all that is needed is that the
// compiler keeps them in program order.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Called by the block's FIRST WAVE only (all 64 lanes of it): no block barrier inside, so the other waves are free to
// do something else meanwhile (the grid search's staging); the caller synchronises the block afterwards.
// Three sections: everything the step reads of the sums and of the OLD state, into registers (with the whole of a gradLM
// step's gates and damped exponential: one lane, rare, and T = dT . T) ; the chain, in registers ; the stores.
__device__ __forceinline__ void step_wave0(IcpState *S, const float *acc, int mode, GradParams gp, float *trace, float *out_T,
                                           int look_slot, float *rec, double *lu_buf, bool solve) {
    __shared__ float sx[6];
    __shared__ float lu_hg[42];  // H | g as the solve saw them, for the pivoted elimination (rare)
    const int t = threadIdx.x;
    // ---- reads
    const float err = S->cur[42], new_err = acc[27], damp0 = S->damp, cur43 = S->cur[43];
    const int it0 = S->it;
    const float lin_t = expand_elem(acc, min(t, 43)), cur_t = S->cur[min(t, 43)];
    const int si = t >> 3, sk = t & 7;
    const bool s_in = si < 6 && sk <= 6;  // the lane holds an element of the augmented system: H (sk < 6) or g (sk = 6)
    const int s_e = s_in ? (sk < 6 ? 6 * si + sk : 36 + si) : 0;
    const float s_new = expand_elem(acc, s_e), s_old = S->cur[s_e];
    const bool lm_accept = new_err < err;
    const bool adopt = mode == STEP_ADOPT || (mode == STEP_LM && lm_accept);
    const float damp1 = (mode == STEP_LM) ? (lm_accept ? damp0 / 2.0f : damp0 * 2.0f) : damp0;
    if (mode == STEP_GRAD_B) {  // the gates and the damped step: a few scalars, one lane
        wave_sync();
        if (t == 0) {
            float diff = new_err - err;
            diff = fminf(fmaxf(diff, -70.0f), 70.0f);
            const float damp_new = gp.lambda_min + gp.range / (1.0f + expf((-gp.B) * diff));
            S->damp = S->damp * damp_new;
            const float sig = 1.0f / powf(1.0f + expf((-gp.B2) * diff), gp.inv_nu);
            for (int i = 0; i < 6; ++i) sx[i] = sig * S->xi[i];
            se3_exp_dev(sx, S->dT);
        }
        wave_sync();
    }
    // T = dT . T  (accepted LM step, every gradLM step): one lane per element, torch.mm's fma chain over k
    const bool mul_T = mode == STEP_GRAD_B || (mode == STEP_LM && lm_accept);
    float new_T = S->T[t & 15];
    if (mul_T) {
        const int i = (t & 15) >> 2, j = t & 3;
        float v = S->dT[4 * i] * S->T[j];
        v = __fmaf_rn(S->dT[4 * i + 1], S->T[4 + j], v);
        v = __fmaf_rn(S->dT[4 * i + 2], S->T[8 + j], v);
        v = __fmaf_rn(S->dT[4 * i + 3], S->T[12 + j], v);
        new_T = v;
    }
    wave_sync();  // the old state has been read
    // ---- the chain: solve, exponential -- in registers; writes xi and dT only (a gradLM step has none: its exponential is above)
    if (solve && mode != STEP_GRAD_B) {  // wave-uniform
        const float h = adopt ? s_new : s_old;
        double a = 0.0;
        if (s_in) a = (double)((sk < 6 && si == sk) ? h + damp1 : h);
        bool ok;
        a = solve6_wave_elim(a, ok);
        const float x_l = (float)a;
        GS_STAMP(14);  // (diagnostic build, wave 0: solved)
        float xi[6];
        if (ok) {  // wave-uniform: every lane saw the same pivots
#pragma unroll
            for (int q = 0; q < 6; ++q) xi[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x_l), 8 * q + 6));
        } else {  // a pivot that is not a positive finite number: the pivoted elimination, on the same H | g and damping
            if (s_in) lu_hg[s_e] = h;
            wave_sync();
            if (t == 0) solve6_lu(lu_hg, lu_hg + 36, damp1, lu_hg + 36, lu_buf);  // (x overwrites g: solve6_lu has copied g by then)
            wave_sync();
#pragma unroll
            for (int q = 0; q < 6; ++q) xi[q] = lu_hg[36 + q];
        }
        const float dT_l = se3_exp_wave(xi);
        float xv = xi[0];
#pragma unroll
        for (int q = 1; q < 6; ++q) xv = t == q ? xi[q] : xv;
        if (t < 6) S->xi[t] = xv;
        if (t < 16) S->dT[t] = dT_l;
    }
    // ---- the bookkeeping: stores
    if (rec) {  // tape: what the look-ahead launch measured, where it wrote, what this step is
        if (t < 44) rec[REC_LIN + t] = lin_t;
        if (t == 44) {
            rec[REC_SLOT] = (float)look_slot;
            rec[REC_MODE] = (float)mode;
            rec[REC_ACCEPT] = (mode == STEP_LM) ? (lm_accept ? 1.0f : 0.0f) : 1.0f;
        }
    }
    if (trace && mode != STEP_ADOPT) {
        float *tr = trace + 48 * it0;
        if (t < 42) tr[t] = cur_t;
        if (t == 42) {
            tr[42] = err; tr[43] = new_err; tr[44] = damp0; tr[45] = (mode == STEP_LM && !lm_accept) ? 0.0f : 1.0f;
            tr[46] = cur43; tr[47] = 0.0f;
        }
    }
    if (adopt && t < 44) S->cur[t] = lin_t;
    if (mul_T && t < 16) S->T[t] = new_T;
    if (t == 0) {
        if (mode != STEP_ADOPT) S->b_first = S->b_cur;  // the neighbour array the iteration's first solve used
        if (adopt) {
            S->p_cur = look_slot >= 0 ? look_slot : 1 - S->p_cur;
            S->b_cur = look_slot >= 0 ? look_slot : 1 - S->b_cur;
        }
        if (mode == STEP_ADOPT) S->b_first = S->b_cur;
        if (mode == STEP_LM) S->damp = damp1;
        if (mode != STEP_ADOPT) S->it = it0 + 1;
    }
    if (out_T && t < 16) out_T[t] = new_T;
    GS_STAMP(13);  // (diagnostic build, wave 0: the books are written -- after 14 on this wave)
    wave_sync();
}

}  // namespace gs
