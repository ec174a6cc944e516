// gs_icp_bwd.hpp -- the reverse pass of the taped ICP loops: kernels and workspace layout (the host driver,
// icp_backward_run, is in icp.hip next to icp_run).  Included by icp.hip.
//
// Gradients (X-bar): the taped loops + a device-side reverse pass.  The reverse pass scatters the adjoints of the
//    associated target points / normals with float atomics (-munsafe-fp-atomics): forward results are bit-stable run
//    to run, those two gradient arrays are not (sums of a few terms per target in arrival order, ~1e-7 relative).
#pragma once

#include "gs_detfold.hpp"
#include "gs_se3_bwd.hpp"

namespace gs {

// ------------------------------------------------------------------ reverse pass of the taped loops
// Walks the tape backwards entirely on the device (accept/reject is read from the records, so rejected LM
// iterations cost two empty launches and no host round trip).  Per iteration:
//   S  small_k  : adjoints of T' = dT T, dT = exp(xi), xi = (H + damp I)^-1 g, and of the gradLM gates
//   B  look_k   : gradLM only -- adjoint of the look-ahead error
//   C  lin_k    : gP_i <- R^T gP_i + adjoint of the linearisation (H, g, e) at s_i ; and, for the step that
//                 produced s from its predecessor cloud q (s = dT q):  sum_i gP_i (x) q_i , sum_i gP_i
//                 -- what the S kernel of that earlier step needs as the adjoint of dT
// gP (ns,3) is updated in place, target / normal adjoints accumulate with float atomics.
constexpr int BWD_MAXB = 512;

struct BwdState {
    float gT[16];    // adjoint of the accumulated transform
    float G[44];     // Hbar(36) | gbar(6) | ebar | pad : what lin_k applies
    float gdT[12];   // adjoint of the top 3 rows of the step being unwound (row-major 3x4)
    float R2[9];     // rotation by which lin_k pulls gP back (the step that produced the cloud gP belongs to)
    float R1[9];     // gradLM: rotation of the look-ahead step
    float gxi[6];
    float g_new_err, g_err, gdamp;
    int active;      // 0: rejected LM iteration, nothing to do
    int src_slot, nn_slot, look_slot;
    int prev_slot;   // slot of the cloud src_slot was derived from (-1: the caller's source cloud)
};

__device__ __forceinline__ const IcpState *rec_state(const float *rec) { return reinterpret_cast<const IcpState *>(rec + REC_STATE); }

// adjoint of one linearised point: returns s_bar, scatters d_bar / n_bar -- or, DET, stores them in row i of this launch's
// contribution rows (g_tgt = those rows, gs_detfold.hpp; NULL: no target adjoint wanted)
template <bool DET = false>
__device__ __forceinline__ f3 lin_point_bwd(const float *G, const Row &r, const f3 s, const uint32_t j, const float *tgt,
                                            const float *nrm, float *g_tgt, float *g_nrm, int i = 0) {
    const f3 d = ld3(tgt, j), n = ld3(nrm, j);
    float ab[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        float v = G[36 + u] * r.b;
#pragma unroll
        for (int w = 0; w < 6; ++w) v += (G[6 * u + w] + G[6 * w + u]) * r.a[w];
        ab[u] = v;
    }
    float bb = 2.0f * G[42] * r.b;
#pragma unroll
    for (int u = 0; u < 6; ++u) bb += G[36 + u] * r.a[u];
    const f3 an{ab[0], ab[1], ab[2]}, ac{ab[3], ab[4], ab[5]};
    f3 sb{n.y * ac.z - n.z * ac.y, n.z * ac.x - n.x * ac.z, n.x * ac.y - n.y * ac.x};
    f3 nb{an.x + (ac.y * s.z - ac.z * s.y), an.y + (ac.z * s.x - ac.x * s.z), an.z + (ac.x * s.y - ac.y * s.x)};
    sb.x -= bb * n.x; sb.y -= bb * n.y; sb.z -= bb * n.z;
    nb.x += bb * (d.x - s.x); nb.y += bb * (d.y - s.y); nb.z += bb * (d.z - s.z);
    if constexpr (DET) {
        if (g_tgt) det_store_row(g_tgt, i, f3{bb * n.x, bb * n.y, bb * n.z}, nb, (int)j);
        return sb;
    }
    if (g_tgt) {
        atomicAdd(g_tgt + 3 * (int64_t)j, bb * n.x);
        atomicAdd(g_tgt + 3 * (int64_t)j + 1, bb * n.y);
        atomicAdd(g_tgt + 3 * (int64_t)j + 2, bb * n.z);
    }
    if (g_nrm) {
        atomicAdd(g_nrm + 3 * (int64_t)j, nb.x);
        atomicAdd(g_nrm + 3 * (int64_t)j + 1, nb.y);
        atomicAdd(g_nrm + 3 * (int64_t)j + 2, nb.z);
    }
    return sb;
}

__device__ __forceinline__ void acc_outer(float *acc, const f3 g, const f3 s) {
    acc[0] += g.x * s.x; acc[1] += g.x * s.y; acc[2] += g.x * s.z; acc[3] += g.x;
    acc[4] += g.y * s.x; acc[5] += g.y * s.y; acc[6] += g.y * s.z; acc[7] += g.y;
    acc[8] += g.z * s.x; acc[9] += g.z * s.y; acc[10] += g.z * s.z; acc[11] += g.z;
}
__device__ __forceinline__ f3 rot_t(const float *R, const f3 g) {  // R^T g, R row-major 3x3
    return f3{R[0] * g.x + R[3] * g.y + R[6] * g.z, R[1] * g.x + R[4] * g.y + R[7] * g.z, R[2] * g.x + R[5] * g.y + R[8] * g.z};
}

// ---- the O(1) steps of the reverse pass, as device functions on a state in LDS (one lane; fp64 where the forward's
// fp32 value would lose the gradient).  They run FOLDED into the prologue of the wide kernel that follows them, the way
// the forward folds its step into the next association: every block recomputes the step from the previous launch's
// outputs (state and partial sums: complete and visible at kernel start), block 0 alone publishes the new state; state
// and partial sums alternate between two buffers from launch to launch.  Per gradLM iteration that is two launches
// instead of four (S1 + look + S2 + lin were 7.3 + 11.4 + 5.7 + 11.6 us, profiles/r03n_fwd_bwd200_kernel_stats.csv).
enum BwdFold { FOLD_G1 = 1, FOLD_G2 = 2, FOLD_LM = 3 };

// S for one LM iteration (record = the STEP_LM record of that iteration)
__device__ void small_lm(BwdState *Sb, const float *rec, const float *__restrict__ rec_global, const float *sums, int iter) {
    const IcpState *S = rec_state(rec);
    if (rec[REC_ACCEPT] == 0.0f) { Sb->active = 0; return; }
    double gdT[12], gxi[6];
    top3_times_Tt(Sb->gT, S->T, gdT);
    for (int k = 0; k < 12; ++k) gdT[k] += (double)sums[k];
    pull_gT(Sb->gT, S->dT);
    se3_exp_bwd(S->xi, gdT, gxi);
    solve_bwd(S->cur, S->damp, S->xi, gxi, Sb->G);
    Sb->G[42] = 0.0f; Sb->G[43] = 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Sb->R2[3 * i + j] = S->dT[4 * i + j];
    Sb->src_slot = S->p_cur; Sb->nn_slot = S->b_cur; Sb->look_slot = (int)rec[REC_SLOT];
    // the cloud of this iteration was made by the closest earlier accepted iteration (from ITS cloud)
    int prev = -1;
    for (int j = iter - 1; j >= 0 && prev < 0; --j) {
        const float *rj = rec_global - (size_t)(iter - j) * REC_WORDS;  // (earlier records: not in the LDS copy)
        if (rj[REC_ACCEPT] != 0.0f) prev = rec_state(rj)->p_cur;
    }
    Sb->prev_slot = prev;
    Sb->active = 1;
}

// S1 for one gradLM iteration (record = its STEP_GRAD_B record; the next record's head = the state after)
__device__ void small_g1(BwdState *Sb, const float *rec, const float *sums, GradParams gp, int prev_slot) {
    const IcpState *S = rec_state(rec), *Sn = rec_state(rec + REC_WORDS);
    const float err = S->cur[42], new_err = rec[REC_LIN + 42];
    const float raw = new_err - err;
    const float diff = fminf(fmaxf(raw, -70.0f), 70.0f);
    const bool pass = raw >= -70.0f && raw <= 70.0f;  // clamp passes the adjoint inside the range (torch.clamp)
    const double eB = exp(-(double)gp.B * diff), eB2 = exp(-(double)gp.B2 * diff);
    const double F = (double)gp.lambda_min + (double)gp.range / (1.0 + eB);
    const double dF = (double)gp.range * (double)gp.B * eB / ((1.0 + eB) * (1.0 + eB));
    const double sig = pow(1.0 + eB2, -(double)gp.inv_nu);
    const double dsig = (double)gp.inv_nu * (double)gp.B2 * eB2 * pow(1.0 + eB2, -(double)gp.inv_nu - 1.0);
    float sx[6];
    for (int i = 0; i < 6; ++i) sx[i] = (float)sig * S->xi[i];
    double gdT2[12], gsx[6];
    top3_times_Tt(Sb->gT, S->T, gdT2);
    for (int k = 0; k < 12; ++k) gdT2[k] += (double)sums[k];
    pull_gT(Sb->gT, Sn->dT);
    se3_exp_bwd(sx, gdT2, gsx);
    double g_s = 0.0;
    for (int i = 0; i < 6; ++i) { g_s += gsx[i] * (double)S->xi[i]; Sb->gxi[i] = (float)(sig * gsx[i]); }
    const double gdamp_next = Sb->gdamp;
    const double g_diff = pass ? gdamp_next * (double)S->damp * dF + g_s * dsig : 0.0;
    Sb->gdamp = (float)(gdamp_next * F);
    Sb->g_new_err = (float)g_diff;
    Sb->g_err = (float)(-g_diff);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { Sb->R2[3 * i + j] = Sn->dT[4 * i + j]; Sb->R1[3 * i + j] = S->dT[4 * i + j]; }
    Sb->src_slot = S->p_cur; Sb->nn_slot = S->b_cur; Sb->look_slot = (int)rec[REC_SLOT];
    Sb->prev_slot = prev_slot;
    Sb->active = 1;
}

// S2: look-ahead step dT1 = exp(xi) -> xi ; then the solve
__device__ void small_g2(BwdState *Sb, const float *rec, const float *sums) {
    const IcpState *S = rec_state(rec);
    double gdT1[12], gxi[6];
    for (int k = 0; k < 12; ++k) gdT1[k] = (double)sums[k];
    se3_exp_bwd(S->xi, gdT1, gxi);
    for (int i = 0; i < 6; ++i) gxi[i] += (double)Sb->gxi[i];
    const double gd = solve_bwd(S->cur, S->damp, S->xi, gxi, Sb->G);
    Sb->gdamp = (float)((double)Sb->gdamp + gd);
    Sb->G[42] = Sb->g_err; Sb->G[43] = 0.0f;
}

// prologue of the wide kernels: the folded small step on an LDS copy of the state; ends with a barrier.
// Everything the step reads -- the state, its tape record with the head of the next one, the partial rows -- is requested in
// ONE batch at kernel start and handed over through LDS: the step runs on one lane, and every global word it used to
// fetch for itself (the record's state, sums, flags: a dozen dependent round trips) is an LDS read now; the rows' loads
// used to follow each other through a four-deep loop (same order of summation as gs_rowsum.hpp's fold_rows with 16 groups: the sums do not change).
__device__ __forceinline__ void bwd_fold(BwdState &sb, const BwdState *__restrict__ Sb_in, BwdState *__restrict__ Sb_out, int fold,
                                         const float *__restrict__ rec, const float *__restrict__ partials_in, int nblocks,
                                         GradParams gp, int arg) {
    __shared__ float sums[12];
    __shared__ float rec_sm[2 * REC_WORDS];
    __shared__ float stage[12][17];
    constexpr int kWords = sizeof(BwdState) / 4, RU = 8;
    static_assert(kWords <= BWD_T, "state copied by one pass of the block");
    static_assert(BWD_T < 2 * REC_WORDS && 2 * REC_WORDS <= 2 * BWD_T, "record pair copied by two loads per thread");
    const int t = threadIdx.x, k = t & 15, g = t >> 4, kc = min(k, 11), last = max(nblocks - 1, 0);
    const int sw = reinterpret_cast<const int *>(Sb_in)[min(t, kWords - 1)];
    const float r0 = rec[t], r1 = rec[BWD_T + min(t, 2 * REC_WORDS - BWD_T - 1)];
    float a[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) a[u] = partials_in[min(g + 16 * u, last) * 12 + kc];
    if (t < kWords) reinterpret_cast<int *>(&sb)[t] = sw;
    rec_sm[t] = r0;
    if (t < 2 * REC_WORDS - BWD_T) rec_sm[BWD_T + t] = r1;
    float v = 0.0f;
#pragma unroll
    for (int u = 0; u < RU; ++u) v += (g + 16 * u < nblocks) ? a[u] : 0.0f;
    for (int b0 = g + 16 * RU; b0 < nblocks; b0 += 16 * RU) {  // (more than 128 rows: further rounds)
#pragma unroll
        for (int u = 0; u < RU; ++u) a[u] = partials_in[min(b0 + 16 * u, last) * 12 + kc];
#pragma unroll
        for (int u = 0; u < RU; ++u) v += (b0 + 16 * u < nblocks) ? a[u] : 0.0f;
    }
    if (k < 12) stage[k][g] = v;
    __syncthreads();
    if (t < 12) {
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) q += stage[t][j];
        sums[t] = q;
    }
    __syncthreads();  // sb, rec_sm and sums are visible
    if (t == 0) {
        if (fold == FOLD_G1) small_g1(&sb, rec_sm, sums, gp, arg);
        else if (fold == FOLD_G2) small_g2(&sb, rec_sm, sums);
        else small_lm(&sb, rec_sm, rec, sums, arg);
    }
    __syncthreads();
    if (blockIdx.x == 0 && t < kWords) reinterpret_cast<int *>(Sb_out)[t] = reinterpret_cast<const int *>(&sb)[t];
}

// B (gradLM), with S1 folded in: adjoint of new_err = e(look, NN(look)); gP_i <- R2^T gP_i + R1^T glook_i ; sums glook (x) s
// (DET: g_tgt = this launch's contribution rows, g_nrm unused -- gs_detfold.hpp)
template <bool DET>
__global__ __launch_bounds__(BWD_T) void bwd_look_k(const BwdState *__restrict__ Sb_in, BwdState *__restrict__ Sb_out,
                                                    const float *__restrict__ rec, const float *__restrict__ partials_in, int nblocks,
                                                    GradParams gp, int prev_slot, LoopBufs B, const int32_t *__restrict__ d_ns,
                                                    const float *__restrict__ tgt, const float *__restrict__ nrm, float thresh,
                                                    float *__restrict__ gP, float *__restrict__ g_tgt, float *__restrict__ g_nrm,
                                                    float *__restrict__ partials) {
    __shared__ BwdState sb;
    __shared__ float G[44];
    bwd_fold(sb, Sb_in, Sb_out, FOLD_G1, rec, partials_in, nblocks, gp, prev_slot);
    if (threadIdx.x < 44) G[threadIdx.x] = (threadIdx.x == 42) ? sb.g_new_err : 0.0f;
    __syncthreads();
    const float *R = sb.R2, *R1 = sb.R1;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
    const float *src = B.P(sb.src_slot), *look = B.P(sb.look_slot);
    const unsigned long long *nn = B.N(sb.look_slot);
    const int ns = *d_ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const Row r = make_row(look, tgt, nrm, nn, i, ns, thresh);
        f3 gl{0.0f, 0.0f, 0.0f};
        if (r.valid) gl = lin_point_bwd<DET>(G, r, ld3(look, i), (uint32_t)(nn[i] & 0xffffffffu), tgt, nrm, g_tgt, g_nrm, i);
        else if (DET && g_tgt) det_store_none(g_tgt, i);
        acc_outer(acc, gl, ld3(src, i));
        const f3 a = rot_t(R, ld3(gP, i)), b = rot_t(R1, gl);
        st3(gP, i, f3{a.x + b.x, a.y + b.y, a.z + b.z});
    }
    block_row<12, BWD_WAVES>(acc, [&](unsigned n) { return &partials[blockIdx.x * 12 + n]; });
}

// C, with S2 (gradLM) or S (LM) folded in: gP_i <- (rotate ? R2^T gP_i : gP_i) + adjoint of (H, g, e) at the iteration's
// source cloud; sums of gP (x) predecessor cloud for the small step of the iteration that made this cloud
// (DET: g_tgt = this launch's contribution rows, g_nrm unused -- gs_detfold.hpp)
template <bool DET>
__global__ __launch_bounds__(BWD_T) void bwd_lin_k(const BwdState *__restrict__ Sb_in, BwdState *__restrict__ Sb_out, int fold,
                                                   const float *__restrict__ rec, const float *__restrict__ partials_in, int nblocks,
                                                   int iter, int rotate, LoopBufs B, const float *__restrict__ user_src,
                                                   const int32_t *__restrict__ d_ns, const float *__restrict__ tgt,
                                                   const float *__restrict__ nrm, float thresh, float *__restrict__ gP,
                                                   float *__restrict__ g_tgt, float *__restrict__ g_nrm,
                                                   float *__restrict__ partials) {
    __shared__ BwdState sb;
    bwd_fold(sb, Sb_in, Sb_out, fold, rec, partials_in, nblocks, GradParams{}, iter);
    if (!sb.active) {  // rejected LM iteration: gP stays as it is, the pending sums are handed on unchanged
        if (threadIdx.x < 12) partials[blockIdx.x * 12 + threadIdx.x] = partials_in[blockIdx.x * 12 + threadIdx.x];
        if (DET && g_tgt)  // no contributions from this launch
            for (int i = blockIdx.x * blockDim.x + threadIdx.x, ns = *d_ns; i < ns; i += gridDim.x * blockDim.x) det_store_none(g_tgt, i);
        return;
    }
    const float *G = sb.G, *R = sb.R2;
    const float *src = B.P(sb.src_slot);
    const float *prev = sb.prev_slot >= 0 ? B.P(sb.prev_slot) : user_src;
    const unsigned long long *nn = B.N(sb.nn_slot);
    const int ns = *d_ns;
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) {
        const Row r = make_row(src, tgt, nrm, nn, i, ns, thresh);
        f3 g = ld3(gP, i);
        if (rotate) g = rot_t(R, g);
        if (r.valid) {
            const f3 sb_ = lin_point_bwd<DET>(G, r, ld3(src, i), (uint32_t)(nn[i] & 0xffffffffu), tgt, nrm, g_tgt, g_nrm, i);
            g.x += sb_.x; g.y += sb_.y; g.z += sb_.z;
        } else if (DET && g_tgt) {
            det_store_none(g_tgt, i);
        }
        st3(gP, i, g);
        acc_outer(acc, g, ld3(prev, i));
    }
    block_row<12, BWD_WAVES>(acc, [&](unsigned n) { return &partials[blockIdx.x * 12 + n]; });
}

struct BwdWs {
    BwdState *S[2];       // double-buffered across launches (bwd_fold)
    float *gP, *partials[2];
};
static inline size_t bwd_ws_layout(int max_ns, void *ws, BwdWs *out) {
    Carve c{(char *)ws};
    BwdWs scratch, &w = out ? *out : scratch;
    w.S[0] = c.take<BwdState>(sizeof(BwdState)); w.S[1] = c.take<BwdState>(sizeof(BwdState));
    w.gP = c.take<float>((size_t)max_ns * 12);
    w.partials[0] = c.take<float>((size_t)BWD_MAXB * 12 * 4); w.partials[1] = c.take<float>((size_t)BWD_MAXB * 12 * 4);
    return c.off;
}

__global__ void zero_rows_k(float *__restrict__ a, float *__restrict__ b, const int32_t *__restrict__ d_n, int cap) {
    const int n = 3 * min(*d_n, cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (a) a[i] = 0.0f;
        if (b) b[i] = 0.0f;
    }
}

// one launch for the reverse pass's preparations: gP and the first partial rows zeroed (nothing depends on the final
// cloud), the target / normal adjoints zeroed over the rows that exist (max_nt may be a generous capacity), the state set
__global__ void bwd_begin_k(BwdState *Sb, const float *__restrict__ grad_T, float *__restrict__ gP, int n_gp, float *__restrict__ partials,
                            int n_part, float *__restrict__ g_tgt, float *__restrict__ g_nrm, const int32_t *__restrict__ d_nt, int cap) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (int i = tid; i < n_gp; i += stride) gP[i] = 0.0f;
    for (int i = tid; i < n_part; i += stride) partials[i] = 0.0f;
    const int n = 3 * min(*d_nt, cap);
    for (int i = tid; i < n; i += stride) {
        if (g_tgt) g_tgt[i] = 0.0f;
        if (g_nrm) g_nrm[i] = 0.0f;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < 16) Sb->gT[threadIdx.x] = grad_T[threadIdx.x];
        if (threadIdx.x == 0) { Sb->gdamp = 0.0f; Sb->active = 0; }
    }
}

// last: through src0 = init_T . user_src; block 0 also adds the last partial sums up into the adjoint of init_T (the T
// chain starts at init_T and src0 = init_T . user_src)
__global__ __launch_bounds__(BWD_T) void bwd_finish_k(const float *__restrict__ init_T, const int32_t *__restrict__ d_ns,
                                                      const float *__restrict__ gP, float *__restrict__ g_src,
                                                      const BwdState *__restrict__ Sb, const float *__restrict__ partials, int nblocks,
                                                      float *__restrict__ g_init_T) {
    __shared__ float R[9];
    __shared__ float sums[12];
    if (threadIdx.x < 9) R[threadIdx.x] = init_T[4 * (threadIdx.x / 3) + threadIdx.x % 3];
    __syncthreads();
    const int ns = *d_ns;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x) st3(g_src, i, rot_t(R, ld3(gP, i)));
    if (blockIdx.x == 0) {  // (block-uniform)
        fold_rows<12, BWD_GROUPS, 16>(partials, nblocks, 12, sums);
        if (threadIdx.x < 16) g_init_T[threadIdx.x] = Sb->gT[threadIdx.x] + (threadIdx.x < 12 ? sums[threadIdx.x] : 0.0f);
    }
}

}  // namespace gs
