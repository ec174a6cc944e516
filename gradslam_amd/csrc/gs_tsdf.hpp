// gs_tsdf.hpp -- what the TSDF volume (tsdf.hip) states once: where a voxel's centre is, what one frame does to one voxel, and
// which grid edges carry a surface point.  The forward integration, its reverse pass and the extraction all read these bodies,
// so that the reverse pass re-takes exactly the forward's decisions and the extraction's normals see the extraction's voxels.
#pragma once

#include "gs_common.hpp"
#include "gs_project.hpp"
#include "gs_rowsum.hpp"

namespace gs {

constexpr int TSDF_T = 256;          // threads per block of every tsdf kernel
constexpr int TSDF_CHUNK = 32;       // frames per integration launch (their cameras sit in LDS; the reverse pass's update mask is 32 bits)
constexpr int TSDF_NMAX = 1 << 29;   // voxels per batch element: edge ids 3 j + a are int32

struct TsdfVol {
    int nx, ny, nz;
    float v, trunc, maxw;
    const float *origin;  // (B, 3) on the device: the corner of voxel (0,0,0)
};
__host__ __device__ __forceinline__ int64_t tsdf_nvox(const TsdfVol &g) { return (int64_t)g.nx * g.ny * g.nz; }

// the chunk [l0, l0 + Lc) of a (B, L) batch of frames
struct TsdfFrames {
    const float *depth, *rgb;  // (B,L,H,W), (B,L,H,W,3); rgb may be NULL
    const float *K, *poses;    // (B,4,4), (B,L,4,4)
    int L, H, W, l0, Lc;
    float umax, vmax;
};

// ------------------------------------------------------------------ the voxel-centre rule
// c_k = o_k + ((float)i_k + 0.5f) * v: one rounded product, one rounded sum (the library is built with -ffp-contract=off)
__device__ __forceinline__ float tsdf_centre1(float o, int i, float v) { return o + ((float)i + 0.5f) * v; }
__device__ __forceinline__ f3 tsdf_centre(const float *__restrict__ o, int ix, int iy, int iz, float v) {
    return f3{tsdf_centre1(o[0], ix, v), tsdf_centre1(o[1], iy, v), tsdf_centre1(o[2], iz, v)};
}
__device__ __forceinline__ void tsdf_unflatten(const TsdfVol &g, int j, int &ix, int &iy, int &iz) {
    const int row = j / g.nx;
    ix = j - row * g.nx;
    iz = row / g.ny;
    iy = row - iz * g.ny;
}

// ------------------------------------------------------------------ the per-frame update
// The chunk's cameras, built by the block's first Lc threads; followed by a barrier.
__device__ __forceinline__ void tsdf_load_cams(Cam *cams, const TsdfFrames &fr, int b, int l0, int Lc) {
    if ((int)threadIdx.x < Lc) cams[threadIdx.x] = make_cam(fr.poses + ((int64_t)b * fr.L + l0 + threadIdx.x) * 16, fr.K + (int64_t)b * 16);
    __syncthreads();
}

// Does frame `depth` (H,W) update the voxel at c?  The three skips: the centre does not project into the image
// (project_point_z, the map's own rule), the pixel holds no depth, the voxel lies more than trunc behind the surface.
__device__ __forceinline__ bool tsdf_observe(const Cam &cam, f3 c, const float *__restrict__ depth, const TsdfFrames &fr, float trunc,
                                             int &pix, float &sdf) {
    int h, w;
    float z;
    if (!project_point_z(cam, c, fr.H, fr.W, fr.umax, fr.vmax, h, w, z)) return false;
    pix = h * fr.W + w;
    const float d = depth[pix];
    if (!(d > 0.0f)) return false;
    sdf = d - z;
    return !(sdf < -trunc);
}
__device__ __forceinline__ float tsdf_sample(float sdf, float trunc) { return fminf(1.0f, sdf / trunc); }
// the running average of tsdf and of every colour component; W is the weight BEFORE the frame
__device__ __forceinline__ float tsdf_average(float W, float old, float t) { return (W * old + t) / (W + 1.0f); }
__device__ __forceinline__ float tsdf_next_weight(float W, float maxw) { return fminf(W + 1.0f, maxw); }
// the weight before a frame that n updates precede (the reverse pass rebuilds it from the update mask): tsdf_next_weight n times
// for the integer-valued weights the integration produces; the cap first applies with the first update
__device__ __forceinline__ float tsdf_weight_after(float W0, int n, float maxw) { return n ? fminf(W0 + (float)n, maxw) : W0; }

// ------------------------------------------------------------------ the edge rule
// edge slot e = 3 j + a runs from voxel j to its +1 neighbour along axis a; it exists iff the neighbour is inside the grid
struct TsdfEdge {
    int j, j1, a;
    int ix, iy, iz;
};
__device__ __forceinline__ bool tsdf_edge(const TsdfVol &g, int64_t e, TsdfEdge &ed) {
    ed.j = (int)(e / 3);
    ed.a = (int)(e - 3 * (int64_t)ed.j);
    tsdf_unflatten(g, ed.j, ed.ix, ed.iy, ed.iz);
    const int i = ed.a == 0 ? ed.ix : (ed.a == 1 ? ed.iy : ed.iz), n = ed.a == 0 ? g.nx : (ed.a == 1 ? g.ny : g.nz);
    if (i + 1 >= n) return false;
    ed.j1 = ed.j + (ed.a == 0 ? 1 : (ed.a == 1 ? g.nx : g.nx * g.ny));
    return true;
}
// both ends observed, and the sign changes (zero counts as outside)
__device__ __forceinline__ bool tsdf_crosses(float f0, float w0, float f1, float w1, float minw) {
    return w0 >= minw && w1 >= minw && ((f0 < 0.0f) != (f1 < 0.0f));
}
__device__ __forceinline__ float tsdf_cross_s(float f0, float f1) { return f0 / (f0 - f1); }

// ------------------------------------------------------------------ the ray-cast rule (tsdf_raycast.hip: forward and reverse)
// Output pixel (i, j) of the strided grid is full-resolution pixel (h, w) = (i s, j s).  Its ray, fp32 in this order:
//   dx = ((float)w - cx) / fx,  dy = ((float)h - cy) / fy,  dw_i = (R_i0 dx + R_i1 dy) + R_i2,
//   len = sqrtf((dx dx + dy dy) + 1),  dz = step / len.
// Sample k (1 <= k < 2^30: the tape is int32) lies at camera depth z_k = (float)k * dz -- one rounded product, never a running
// sum, so the reverse pass and a reference find sample k without walking the ray -- at p_i = t_i + z_k dw_i, and belongs to
// the ray iff near <= z_k <= far.  Consecutive samples are exactly `step` apart in space.
struct TsdfRay {
    f3 t, dw;
    float dz;
};
// the ray's camera direction (dx, dy, 1) of full-resolution pixel (h, w)
__device__ __forceinline__ void tsdf_ray_dir(const float *__restrict__ K, int h, int w, float &dx, float &dy) {
    dx = ((float)w - K[2]) / K[0];
    dy = ((float)h - K[6]) / K[5];
}
__device__ __forceinline__ TsdfRay tsdf_ray(const float *__restrict__ K, const float *__restrict__ P, int h, int w, float step) {
    float dx, dy;
    tsdf_ray_dir(K, h, w, dx, dy);
    TsdfRay r;
    r.t = f3{P[3], P[7], P[11]};
    r.dw = f3{(P[0] * dx + P[1] * dy) + P[2], (P[4] * dx + P[5] * dy) + P[6], (P[8] * dx + P[9] * dy) + P[10]};
    r.dz = step / sqrtf((dx * dx + dy * dy) + 1.0f);
    return r;
}
__device__ __forceinline__ float tsdf_ray_z(const TsdfRay &r, int k) { return (float)k * r.dz; }
__device__ __forceinline__ f3 tsdf_ray_at(const TsdfRay &r, float z) { return f3{r.t.x + z * r.dw.x, r.t.y + z * r.dw.y, r.t.z + z * r.dw.z}; }

// The cell of a position: per axis g = (p - o) / v - 0.5f, i = floorf(g), a = g - i; inside iff 0 <= i and i + 1 <= n - 1 on all
// three axes (the 8 corners i, i + 1 exist).  Written so that a NaN or an infinity is outside; every gather below follows it.
struct TsdfCell {
    int j;  // the corner (ix, iy, iz) within one batch element
    float ax, ay, az;
};
__device__ __forceinline__ bool tsdf_cell1(float p, float o, float v, int n, int &i, float &a) {
    const float g = (p - o) / v - 0.5f, fi = floorf(g);
    if (!(fi >= 0.0f && fi + 1.0f <= (float)(n - 1))) return false;
    i = (int)fi;
    a = g - fi;
    return true;
}
__device__ __forceinline__ bool tsdf_cell(const TsdfVol &g, const float *__restrict__ o, f3 p, TsdfCell &c) {
    int ix, iy, iz;
    if (!tsdf_cell1(p.x, o[0], g.v, g.nx, ix, c.ax) || !tsdf_cell1(p.y, o[1], g.v, g.ny, iy, c.ay) ||
        !tsdf_cell1(p.z, o[2], g.v, g.nz, iz, c.az))
        return false;
    c.j = (iz * g.ny + iy) * g.nx + ix;
    return true;
}
// corner c = x + 2 y + 4 z of the cell at j
__device__ __forceinline__ int tsdf_corner(const TsdfVol &g, int j, int c) {
    return j + (c & 1) + ((c >> 1) & 1) * g.nx + (c >> 2) * g.nx * g.ny;
}
// observed iff all 8 corner weights are >= minw (tested before the 8 tsdf values are fetched: unobserved space costs half)
__device__ __forceinline__ bool tsdf_cell_observed(const TsdfVol &g, const float *__restrict__ weight, int j, float minw) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && weight[tsdf_corner(g, j, c)] >= minw;
    return ok;
}
__device__ __forceinline__ float tsdf_lerp(float p, float q, float s) { return p + s * (q - p); }
// four times along x, twice along y, once along z
__device__ __forceinline__ float tsdf_trilerp(const float *f, const TsdfCell &c) {
    const float c00 = tsdf_lerp(f[0], f[1], c.ax), c10 = tsdf_lerp(f[2], f[3], c.ax);
    const float c01 = tsdf_lerp(f[4], f[5], c.ax), c11 = tsdf_lerp(f[6], f[7], c.ax);
    return tsdf_lerp(tsdf_lerp(c00, c10, c.ay), tsdf_lerp(c01, c11, c.ay), c.az);
}
// the gradient of the interpolant in voxel units: differences along the axis, lerped over the other two (x before y before z)
__device__ __forceinline__ f3 tsdf_trigrad(const float *f, const TsdfCell &c) {
    const float gx = tsdf_lerp(tsdf_lerp(f[1] - f[0], f[3] - f[2], c.ay), tsdf_lerp(f[5] - f[4], f[7] - f[6], c.ay), c.az);
    const float gy = tsdf_lerp(tsdf_lerp(f[2] - f[0], f[3] - f[1], c.ax), tsdf_lerp(f[6] - f[4], f[7] - f[5], c.ax), c.az);
    const float gz = tsdf_lerp(tsdf_lerp(f[4] - f[0], f[5] - f[1], c.ax), tsdf_lerp(f[6] - f[2], f[7] - f[3], c.ax), c.ay);
    return f3{gx, gy, gz};
}
// the weight of corner c in the interpolant: (wx wy) wz with w = a at the far end of an axis, 1 - a at the near end
__device__ __forceinline__ float tsdf_corner_weight(const TsdfCell &c, int k) {
    const float wx = (k & 1) ? c.ax : 1.0f - c.ax, wy = (k & 2) ? c.ay : 1.0f - c.ay, wz = (k & 4) ? c.az : 1.0f - c.az;
    return (wx * wy) * wz;
}
__device__ __forceinline__ void tsdf_gather8(const TsdfVol &g, const float *__restrict__ x, int j, float *f) {
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = x[tsdf_corner(g, j, c)];
}
__device__ __forceinline__ void tsdf_gather8c(const TsdfVol &g, const float *__restrict__ col, int j, int ch, float *f) {
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = col[3 * (int64_t)tsdf_corner(g, j, c) + ch];
}
// One sample of one batch element's volume: observed -> its value.
__device__ __forceinline__ bool tsdf_sample_at(const TsdfVol &g, const float *__restrict__ o, const float *__restrict__ tsdf,
                                               const float *__restrict__ weight, float minw, f3 p, TsdfCell &c, float &f) {
    if (!tsdf_cell(g, o, p, c) || !tsdf_cell_observed(g, weight, c.j, minw)) return false;
    float f8[8];
    tsdf_gather8(g, tsdf, c.j, f8);
    f = tsdf_trilerp(f8, c);
    return true;
}
// The march ends at the first observed sample k with f < 0 (zero counts as outside, as in tsdf_crosses); it is a hit iff sample
// k - 1 belongs to the ray, is observed and has f_prev >= 0.  Then s = f_prev / (f_prev - f), z* = ((float)(k - 1) + s) dz,
// p* = t + z* dw, and p* must be observed too.
__device__ __forceinline__ bool tsdf_hit_at(const TsdfVol &g, const float *__restrict__ o, const float *__restrict__ weight, float minw,
                                            const TsdfRay &r, int k, float f_prev, float f, float &z, TsdfCell &c) {
    const float s = f_prev / (f_prev - f);
    z = ((float)(k - 1) + s) * r.dz;
    return tsdf_cell(g, o, tsdf_ray_at(r, z), c) && tsdf_cell_observed(g, weight, c.j, minw);
}

// ------------------------------------------------------------------ the pose sums of the reverse passes (integration and cast)
// A camera's pose adjoint is N sums over the threads of many blocks (integration: N = 4 over the voxels, cast: N = 12 over the
// pixels).  Plain fp32 in gs_rowsum.hpp's fixed order, no atomics, so the same bits from run to run:
//   1. tsdf_pose_wave: the wave's butterflies.  `on`: this lane holds terms (else its x must be +0).  A wave without any skips
//      the butterfly and leaves +0 (what the butterfly of 64 +0 gives).  tsdf_bwd_k keeps one set of wave sums per frame of a chunk.
//   2. block_row_sum<N, TSDF_WAVES> behind a barrier: one row of N per block and camera.
//   3. fold_rows<N, TSDF_POSE_GROUPS, 16> in the finishing launch, TSDF_POSE_T threads per camera.
constexpr int TSDF_WAVES = TSDF_T / kWave;
constexpr int TSDF_POSE_T = 1024, TSDF_POSE_GROUPS = TSDF_POSE_T / 16;
template <int N>
__device__ __forceinline__ void tsdf_pose_wave(const float (&x)[N], bool on, float *__restrict__ red) {  // red: [TSDF_WAVES][N]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool any = __ballot(on) != 0ull;  // wave-uniform: every lane of the wave arrives here
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float s = any ? wave_sum(x[n]) : 0.0f;
        if (lane == 0) red[wave * N + n] = s;
    }
}

}  // namespace gs
