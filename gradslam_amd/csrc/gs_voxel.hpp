// gs_voxel.hpp -- the rules of the voxel downsample that voxel.hip's kernels and its host entry points share: the voxel key of
// a point, the hash table's shape, and the two workspace layouts (each stated once: size query and carving run the same code).
//
// Clouds come as the renderer and the metrics take them: points (B, N_max, 3) fp32, padded, with (B,) int32 device counts.
#pragma once
#include "gs_common.hpp"
#include "gs_fixed128.hpp"

namespace gs {

constexpr int VOX_T = 256;                          // threads per block of the row-parallel kernels
constexpr int VOX_NMAX = 1 << 29;                   // rows per batch element at most: the table then has 2^30 slots
constexpr int VOX_CMAX = 64;                        // components per attribute at most
constexpr int VOX_KBIAS = 1 << 20;                  // |k| < 2^20 per axis: 21 biased bits, three axes in 63
constexpr unsigned long long VOX_EMPTY = ~0ull;     // bit 63 set: no valid key

// slots per batch element: the smallest power of two >= 2 N_max (load <= 0.5)
static inline int64_t vox_slots(int N_max) {
    int64_t s = 1;
    while (s < 2 * (int64_t)N_max) s <<= 1;
    return s;
}
static inline int vox_blocks(int N_max) { return cdiv(N_max, 1024); }  // = compact_blocks(N_max): rows per compaction block

// The voxel of a point: k = floorf((p - o) / v) per axis, one fp32 subtraction and one IEEE fp32 division (no fast-math, no
// contraction).  False for a non-finite coordinate and for |k| >= 2^20 on any axis (a NaN or infinite quotient included).
__device__ __forceinline__ bool vox_key(const f3 p, const f3 o, float v, unsigned long long &key) {
    const float kx = floorf((p.x - o.x) / v), ky = floorf((p.y - o.y) / v), kz = floorf((p.z - o.z) / v);
    const float lim = (float)VOX_KBIAS;
    const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
    if (!(finite && fabsf(kx) < lim && fabsf(ky) < lim && fabsf(kz) < lim)) return false;
    const unsigned long long bx = (unsigned long long)((int)kx + VOX_KBIAS), by = (unsigned long long)((int)ky + VOX_KBIAS),
                             bz = (unsigned long long)((int)kz + VOX_KBIAS);
    key = bx | (by << 21) | (bz << 42);
    return true;
}

// first probe position (the finaliser of splitmix64: neighbouring voxels land far apart)
__device__ __forceinline__ uint32_t vox_hash(unsigned long long k, uint32_t mask) {
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return (uint32_t)k & mask;
}

// ------------------------------------------------------------------ workspace of gs_voxel_assign
struct VoxWs {
    int32_t *err;               // 1: set when a probe sequence ran through the whole table (a bug: the load is <= 0.5)
    unsigned long long *keys;   // (B, S) the table's keys, VOX_EMPTY = free
    uint32_t *rows;             // (B, S) lowest member row of the slot's voxel
    int32_t *slot;              // (B, N_max) the slot of every row; < 0: no voxel (padding -1, dropped -2)
    int *bcount, *boffset;      // (B, nb) each: the compaction's per-block counts and their exclusive scan
    int64_t S;
    int nb;
};
static size_t vox_assign_layout(int B, int N_max, void *ws, VoxWs *out) {
    Carve c{(char *)ws};
    VoxWs scratch, &r = out ? *out : scratch;
    r.S = vox_slots(N_max);
    r.nb = vox_blocks(N_max);
    r.err = c.take<int32_t>(4);
    r.keys = c.take<unsigned long long>((size_t)B * r.S * 8);
    r.rows = c.take<uint32_t>((size_t)B * r.S * 4);
    r.slot = c.take<int32_t>((size_t)B * N_max * 4);
    r.bcount = c.take<int>((size_t)B * r.nb * 4);
    r.boffset = c.take<int>((size_t)B * r.nb * 4);
    return c.off;
}

// ------------------------------------------------------------------ workspace of gs_voxel_reduce (zeroed as one piece): the
// fold of gs_fixed128.hpp over B M_max rows of C sums
static size_t vox_reduce_layout(int B, int M_max, int C, void *ws, Fold *out) {
    Carve c{(char *)ws};
    const Fold f = fold_carve(c, (size_t)B * M_max, C, true);  // sums | flags | maximum
    if (out) *out = f;
    return c.off;
}

}  // namespace gs
