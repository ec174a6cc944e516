// gs_tsdf.hpp -- what the TSDF volume (tsdf.hip) states once: where a voxel's centre is, what one frame does to one voxel, and
// which grid edges carry a surface point.  The forward integration, its reverse pass and the extraction all read these bodies,
// so that the reverse pass re-takes exactly the forward's decisions and the extraction's normals see the extraction's voxels.
#pragma once

#include "gs_common.hpp"
#include "gs_project.hpp"

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

}  // namespace gs
