// Surface nets on the live 8 x 8 x 8 bricks of a lattice (include/perf_hip_brickmesh.h): select -> list -> corners -> count -> scan ->
// write, no case tables, no atomics.
//
// A SLAB is one x-layer of a brick: 8 x 8 cells, lanes (j, k) = (lane >> 3, lane & 7) of one wave, word 8 slot + i.  The count pass
// needs only inside bits: the slab's own corner layer and the layer above it are one coalesced 256-byte load and a ballot each, the
// 2 x 17 corners on the +y / +z faces of the neighbour bricks (found through the table) are one more load by 34 lanes; active cells and
// quads are 64-bit mask arithmetic on wave-uniform values.  The write pass classifies a slab again BY THE SAME FUNCTION, so both passes
// skip the same quads, and touches corner values only where a cell is active.
#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_scan_device.hpp"
#include "../../include/perf_hip_brickmesh.h"

namespace perf {

constexpr uint64_t kRow0 = 0xffull;                      // cells / corners with j == 0
constexpr uint64_t kCol0 = 0x0101010101010101ull;        // cells / corners with k == 0

struct BrickDims {
    int32_t nx, ny, nz;              // cells
    int32_t bx, by, bz;              // bricks
    int32_t m;                       // live bricks
};

// ---- which bricks are live --------------------------------------------------------------------------------------------------------------
// x01 of lattice corner i of n: fl32(fl32(i) * fl32(1 / n)) -- what density_lattice's `ijk.float() / float(res)` evaluates to on the
// device (a tensor divided by a host scalar is multiplied by the scalar's fp32 reciprocal), so that the corners' bits are its bits; the
// correctly rounded i / n where n is a power of two.  The occupancy cell of the corner: int(clip(x01, 0.0005, 0.9995) * R) in fp32.
__device__ __forceinline__ float bm_x01(int32_t i, int32_t n) { return mul_rn((float)i, __fdiv_rn(1.0f, (float)n)); }
__device__ __forceinline__ int32_t bm_occ_cell(float x, int32_t occ_res) {
    const float c = x < 0.0005f ? 0.0005f : (x > 0.9995f ? 0.9995f : x);
    const int32_t cell = (int32_t)mul_rn(c, (float)occ_res);
    return cell < 0 ? 0 : (cell > occ_res - 1 ? occ_res - 1 : cell);          // (never outside the grid, whatever R)
}

// One thread per brick; a workgroup's 256 bricks get their rank within the group, the group's live count goes to sums[group].
__global__ void __launch_bounds__(256) brickmesh_select_kernel(const uint8_t* __restrict__ binaries, int32_t occ_res, BrickDims d, int64_t n_bricks_all,
                                                               int32_t* __restrict__ table, uint64_t* __restrict__ sums) {
    __shared__ int32_t wave_sum[4];
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool live = false;
    if (b < n_bricks_all) {
        const int32_t cz = (int32_t)(b % d.bz), cy = (int32_t)((b / d.bz) % d.by), cx = (int32_t)(b / ((int64_t)d.bz * d.by));
        const int32_t x0 = bm_occ_cell(bm_x01(8 * cx, d.nx), occ_res), x1 = bm_occ_cell(bm_x01(min(8 * cx + 8, d.nx), d.nx), occ_res);
        const int32_t y0 = bm_occ_cell(bm_x01(8 * cy, d.ny), occ_res), y1 = bm_occ_cell(bm_x01(min(8 * cy + 8, d.ny), d.ny), occ_res);
        const int32_t z0 = bm_occ_cell(bm_x01(8 * cz, d.nz), occ_res), z1 = bm_occ_cell(bm_x01(min(8 * cz + 8, d.nz), d.nz), occ_res);
        for (int32_t x = x0; x <= x1 && !live; ++x)
            for (int32_t y = y0; y <= y1 && !live; ++y) {
                const uint8_t* row = binaries + ((int64_t)x * occ_res + y) * occ_res;
                for (int32_t z = z0; z <= z1; ++z) live = live || row[z] != 0;
            }
    }
    const uint64_t mask = __ballot(live);
    if (lane == 0) wave_sum[wave] = __popcll(mask);
    __syncthreads();
    int32_t before = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    if (b < n_bricks_all) table[b] = live ? before + __popcll(mask & ((1ull << lane) - 1)) : -1;
    if (threadIdx.x == 0) sums[blockIdx.x] = (uint64_t)total;
}

__global__ void __launch_bounds__(256) brickmesh_select_add_kernel(int32_t* __restrict__ table, int64_t n_bricks_all, const uint64_t* __restrict__ prefix,
                                                                   const uint64_t* __restrict__ total, int64_t* __restrict__ n_live_dev) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b < n_bricks_all) {
        const int32_t s = table[b];
        if (s >= 0) table[b] = s + (int32_t)prefix[blockIdx.x];
    }
    if (b == 0) n_live_dev[0] = (int64_t)total[0];
}

__global__ void __launch_bounds__(256) brickmesh_list_kernel(const int32_t* __restrict__ table, int64_t n_bricks_all, int32_t* __restrict__ ids, int32_t n_bricks) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_bricks_all) return;
    const int32_t s = table[b];
    if (s >= 0 && s < n_bricks) ids[s] = (int32_t)b;
}

// One thread per stored corner of the slots first .. first + m - 1.
__global__ void __launch_bounds__(256) brickmesh_corners_kernel(const int32_t* __restrict__ ids, int32_t first, int64_t n_corners, BrickDims d, int64_t n_bricks_all,
                                                                const uint8_t* __restrict__ binaries, int32_t occ_res, float* __restrict__ x01,
                                                                uint8_t* __restrict__ sel, uint8_t* __restrict__ interior) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_corners) return;
    int64_t b = ids[first + (t >> 9)];
    b = b < 0 ? 0 : (b > n_bricks_all - 1 ? n_bricks_all - 1 : b);
    const int32_t cz = (int32_t)(b % d.bz), cy = (int32_t)((b / d.bz) % d.by), cx = (int32_t)(b / ((int64_t)d.bz * d.by));
    const int32_t local = (int32_t)(t & 511);
    const float x = bm_x01(8 * cx + (local >> 6), d.nx), y = bm_x01(8 * cy + ((local >> 3) & 7), d.ny), z = bm_x01(8 * cz + (local & 7), d.nz);
    x01[3 * t] = x; x01[3 * t + 1] = y; x01[3 * t + 2] = z;
    const bool in = x > 0.f && x < 1.f && y > 0.f && y < 1.f && z > 0.f && z < 1.f;
    const bool occ = binaries[((int64_t)bm_occ_cell(x, occ_res) * occ_res + bm_occ_cell(y, occ_res)) * occ_res + bm_occ_cell(z, occ_res)] != 0;
    sel[t] = (in && occ) ? 1 : 0;
    if (interior) interior[t] = in ? 1 : 0;
}

// ---- a slab's classification ------------------------------------------------------------------------------------------------------------
struct BrickSet {
    const float* values;             // [m, 512]
    const int32_t* ids;              // [m]
    const int32_t* table;            // [bx, by, bz]
};

struct Slab {
    uint64_t active, qx, qy, qz;     // cells with a vertex; corners p whose edge along x / y / z emits a quad (violations taken out)
    uint32_t violations;
    int32_t cx, cy, cz;              // the brick
};

// lane t < 27 holds the slot of the brick at offset (t / 9 - 1, t / 3 % 3 - 1, t % 3 - 1) from (cx, cy, cz): -1 where there is none
// (outside the lattice, or not live); slots are clamped below m
__device__ __forceinline__ int32_t bm_neighbour_slots(const int32_t* __restrict__ table, const BrickDims& d, int32_t cx, int32_t cy, int32_t cz, int32_t lane) {
    const int32_t t = lane < 27 ? lane : 13;
    const int32_t x = cx + t / 9 - 1, y = cy + (t / 3) % 3 - 1, z = cz + t % 3 - 1;
    const bool inside = x >= 0 && x < d.bx && y >= 0 && y < d.by && z >= 0 && z < d.bz;
    const int32_t s = table[inside ? ((int64_t)x * d.by + y) * d.bz + z : ((int64_t)cx * d.by + cy) * d.bz + cz];
    return inside ? (s < d.m ? s : d.m - 1) : -1;
}

// (dx, dy, dz) in {-1, 0, 1}: wave-uniform
__device__ __forceinline__ int32_t bm_nbr(int32_t nb, int dx, int dy, int dz) { return __builtin_amdgcn_readlane(nb, (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)); }

// bit j of an 8-bit value -> bit 8 j
__device__ __forceinline__ uint64_t bm_spread8(uint64_t x) {
    x = (x | (x << 28)) & 0x0000000f0000000full;
    x = (x | (x << 14)) & 0x0003000300030003ull;
    x = (x | (x << 7)) & 0x0101010101010101ull;
    return x;
}

// All 64 lanes of the wave arrive.  w = 8 slot + i.
__device__ __forceinline__ Slab bm_classify(const BrickSet& set, const BrickDims& d, float thr, float fill, int64_t w, int32_t lane, int32_t& nb_out) {
    Slab r;
    const int32_t slot = (int32_t)(w >> 3), li = (int32_t)(w & 7);
    const int64_t n_all = (int64_t)d.bx * d.by * d.bz;
    int64_t b = set.ids[slot];
    b = b < 0 ? 0 : (b > n_all - 1 ? n_all - 1 : b);
    r.cz = (int32_t)(b % d.bz); r.cy = (int32_t)((b / d.bz) % d.by); r.cx = (int32_t)(b / ((int64_t)d.bz * d.by));
    const int32_t nb = bm_neighbour_slots(set.table, d, r.cx, r.cy, r.cz, lane);
    nb_out = nb;
    // the slab's own corner layer, the layer above it (the +x brick's layer 0 behind the brick's last slab), and on lanes 0 .. 33 the
    // 17 corners of each of the two layers that the +y / +z / +y+z bricks hold: (8, k), (j, 8), (8, 8)
    const float* own = set.values + (int64_t)slot * 512;
    const int32_t sx = li == 7 ? bm_nbr(nb, 1, 0, 0) : slot;
    const float v0 = own[li * 64 + lane];
    const float v1l = set.values[(int64_t)(sx < 0 ? 0 : sx) * 512 + ((li + 1) & 7) * 64 + lane];
    const float v1 = sx < 0 ? fill : v1l;
    const int32_t e = lane < 34 ? lane : 0, plane = e / 17, q = e % 17;
    const int32_t ej = q < 8 ? 8 : (q < 16 ? q - 8 : 8), ek = q < 8 ? q : 8, ei = li + plane;
    const int32_t es = __shfl(nb, 13 + 9 * (ei >> 3) + 3 * (ej >> 3) + (ek >> 3));
    const float vel = set.values[(int64_t)(es < 0 ? 0 : es) * 512 + ((ei & 7) * 8 + (ej & 7)) * 8 + (ek & 7)];
    const float ve = es < 0 ? fill : vel;
    const uint64_t m0 = __ballot(v0 >= thr), m1 = __ballot(v1 >= thr), ex = __ballot(lane < 34 && ve >= thr);
    uint64_t mz[2], my[2], myz[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint64_t m = p ? m1 : m0;
        const uint64_t yrow = (ex >> (17 * p)) & 0xff, zcol = (ex >> (17 * p + 8)) & 0xff, corner = (ex >> (17 * p + 16)) & 1;
        mz[p] = ((m >> 1) & 0x7f7f7f7f7f7f7f7full) | (bm_spread8(zcol) << 7);           // corner (j, k + 1)
        my[p] = (m >> 8) | (yrow << 56);                                                  // corner (j + 1, k)
        myz[p] = (mz[p] >> 8) | (((yrow >> 1) | (corner << 7)) << 56);                    // corner (j + 1, k + 1)
    }
    const uint64_t all = m0 & mz[0] & my[0] & myz[0] & m1 & mz[1] & my[1] & myz[1];
    const uint64_t any = m0 | mz[0] | my[0] | myz[0] | m1 | mz[1] | my[1] | myz[1];
    r.active = any & ~all;
    // the three lattice edges that start at corner p = the cell's corner 0: along x (needs j, k >= 1), y (k, i >= 1), z (i, j >= 1)
    const uint64_t j_ge1 = r.cy == 0 ? ~kRow0 : ~0ull, k_ge1 = r.cz == 0 ? ~kCol0 : ~0ull;
    const bool i_ge1 = r.cx > 0 || li > 0;
    uint64_t qx = (m0 ^ m1) & j_ge1 & k_ge1;
    uint64_t qy = i_ge1 ? ((m0 ^ my[0]) & k_ge1) : 0;
    uint64_t qz = i_ge1 ? ((m0 ^ mz[0]) & j_ge1) : 0;
    // a quad needs the cells p, p - e_b, p - e_c, p - e_b - e_c: where one of them lies in a brick that is not live, a violation
    const bool no_x = li == 0 && bm_nbr(nb, -1, 0, 0) < 0, no_y = bm_nbr(nb, 0, -1, 0) < 0, no_z = bm_nbr(nb, 0, 0, -1) < 0;
    const bool no_xy = li == 0 && bm_nbr(nb, -1, -1, 0) < 0, no_xz = li == 0 && bm_nbr(nb, -1, 0, -1) < 0, no_yz = bm_nbr(nb, 0, -1, -1) < 0;
    const uint64_t vx = qx & ((no_y ? kRow0 : 0) | (no_z ? kCol0 : 0) | (no_yz ? 1ull : 0));
    const uint64_t vy = qy & ((no_z ? kCol0 : 0) | (no_x ? ~0ull : 0) | (no_xz ? kCol0 : 0));
    const uint64_t vz = qz & ((no_y ? kRow0 : 0) | (no_x ? ~0ull : 0) | (no_xy ? kRow0 : 0));
    r.qx = qx & ~vx; r.qy = qy & ~vy; r.qz = qz & ~vz;
    uint32_t violations = __popcll(vx) + __popcll(vy) + __popcll(vz);
    // and the edges that END at a stored corner of this slab and start in a brick that is not live (there p is `fill`: outside)
    if (no_x && r.cx > 0) violations += __popcll(m0 & j_ge1 & k_ge1);
    if (no_y && r.cy > 0 && i_ge1) violations += __popcll(m0 & kRow0 & k_ge1);
    if (no_z && r.cz > 0 && i_ge1) violations += __popcll(m0 & kCol0 & j_ge1);
    r.violations = violations;
    return r;
}

__global__ void __launch_bounds__(256) brickmesh_count_kernel(BrickSet set, BrickDims d, float thr, float fill, int64_t n_slabs, uint64_t* __restrict__ masks,
                                                              uint64_t* __restrict__ ranks, uint64_t* __restrict__ violations) {
    const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= n_slabs) return;                       // (wave-uniform)
    const int32_t lane = threadIdx.x & 63;
    int32_t nb;
    const Slab s = bm_classify(set, d, thr, fill, w, lane, nb);
    if (lane == 0) {
        masks[w] = s.active;
        ranks[w] = ((uint64_t)(__popcll(s.qx) + __popcll(s.qy) + __popcll(s.qz)) << 32) | (uint64_t)__popcll(s.active);
        violations[w] = s.violations;
    }
}

// the two scans' totals, unpacked: (vertices, triangles, violations) to the workspace and to the caller
__global__ void brickmesh_totals_kernel(const uint64_t* __restrict__ packed, const uint64_t* __restrict__ violations, int64_t* __restrict__ totals_ws,
                                        int64_t* __restrict__ counts_dev) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t v = packed ? (int64_t)(packed[0] & 0xffffffffull) : 0, t = packed ? 2 * (int64_t)(packed[0] >> 32) : 0;
    const int64_t bad = violations ? (int64_t)violations[0] : 0;
    totals_ws[0] = v; totals_ws[1] = t; totals_ws[2] = bad; totals_ws[3] = 0;
    counts_dev[0] = v; counts_dev[1] = t; counts_dev[2] = bad;
}

// eight wave-uniform slots, one per offset 4 dx + 2 dy + dz (named members: they stay in scalar registers)
struct Slots8 {
    int32_t s0, s1, s2, s3, s4, s5, s6, s7;
    __device__ __forceinline__ int32_t pick(int32_t which) const {
        int32_t slot = s0;
        slot = which == 1 ? s1 : slot; slot = which == 2 ? s2 : slot; slot = which == 3 ? s3 : slot; slot = which == 4 ? s4 : slot;
        slot = which == 5 ? s5 : slot; slot = which == 6 ? s6 : slot; slot = which == 7 ? s7 : slot;
        return slot;
    }
};

// the bricks at sign * (dx, dy, dz) of the brick whose 27 neighbour slots the lanes of nb hold
__device__ __forceinline__ Slots8 bm_slots8(int32_t nb, int sign) {
    return Slots8{bm_nbr(nb, 0, 0, 0),    bm_nbr(nb, 0, 0, sign),    bm_nbr(nb, 0, sign, 0),    bm_nbr(nb, 0, sign, sign),
                  bm_nbr(nb, sign, 0, 0), bm_nbr(nb, sign, 0, sign), bm_nbr(nb, sign, sign, 0), bm_nbr(nb, sign, sign, sign)};
}

// the value of corner (i, j, k) in 0 .. 8 of the brick whose 2 x 2 x 2 UPPER neighbourhood of slots is s
__device__ __forceinline__ float bm_corner(const float* __restrict__ values, const Slots8& s, float fill, int32_t i, int32_t j, int32_t k) {
    const int32_t slot = s.pick(4 * (i >> 3) + 2 * (j >> 3) + (k >> 3));
    const float v = values[(int64_t)(slot < 0 ? 0 : slot) * 512 + ((i & 7) * 8 + (j & 7)) * 8 + (k & 7)];
    return slot < 0 ? fill : v;
}

// the rank of the vertex of cell (i, j, k) in -1 .. 7 of the brick whose 2 x 2 x 2 LOWER neighbourhood of slots is s (offset 4: the
// brick at -x); only asked for cells whose brick is live
__device__ __forceinline__ int32_t bm_rank(const uint64_t* __restrict__ masks, const uint64_t* __restrict__ ranks, const Slots8& s, int32_t i, int32_t j, int32_t k) {
    const int32_t slot = s.pick(4 * (i < 0) + 2 * (j < 0) + (k < 0));
    const int64_t w = (int64_t)(slot < 0 ? 0 : slot) * 8 + (i & 7);
    return (int32_t)(ranks[w] & 0xffffffffull) + __popcll(masks[w] & ((1ull << ((j & 7) * 8 + (k & 7))) - 1));
}

// The quad of the lattice edge from corner p = (i, j, k) of the brick along axis A, as triangle rows 2 quad and 2 quad + 1: the vertices of
// the cells p - e_b - e_c, p - e_c, p, p - e_b (b = A + 1, c = A + 2 mod 3), reversed when p is outside.
template <int A>
__device__ __forceinline__ void bm_emit_quad(const uint64_t* __restrict__ masks, const uint64_t* __restrict__ ranks, const Slots8& down, int32_t i, int32_t j, int32_t k,
                                             bool p_inside, int64_t quad, int32_t* __restrict__ faces, int64_t face_capacity) {
    constexpr int B = (A + 1) % 3, C = (A + 2) % 3;
    constexpr int bi = B == 0, bj = B == 1, bk = B == 2, ci = C == 0, cj = C == 1, ck = C == 2;
    int32_t q0 = bm_rank(masks, ranks, down, i - bi - ci, j - bj - cj, k - bk - ck);
    int32_t q1 = bm_rank(masks, ranks, down, i - ci, j - cj, k - ck);
    int32_t q2 = bm_rank(masks, ranks, down, i, j, k);
    int32_t q3 = bm_rank(masks, ranks, down, i - bi, j - bj, k - bk);
    if (!p_inside) { const int32_t t0 = q0, t1 = q1; q0 = q3; q1 = q2; q2 = t1; q3 = t0; }
    const int64_t tri = 2 * quad;
    if (tri + 1 < face_capacity) {
        int32_t* f = faces + 3 * tri;
        f[0] = q0; f[1] = q1; f[2] = q2;
        f[3] = q0; f[4] = q2; f[5] = q3;
    }
}

// A wave takes 64 consecutive slabs: their masks are one coalesced load, and only the slabs with an active cell are visited (a slab
// without one has neither a vertex nor a quad: an edge with differing ends makes its four cells active).
__global__ void __launch_bounds__(256) brickmesh_write_kernel(BrickSet set, BrickDims d, float thr, float fill, MeshBox box, int64_t n_slabs,
                                                              const uint64_t* __restrict__ masks, const uint64_t* __restrict__ ranks, float* __restrict__ vertices,
                                                              int64_t vertex_capacity, int32_t* __restrict__ faces, int64_t face_capacity, int64_t* __restrict__ cells) {
    const int64_t first = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 64;
    if (first >= n_slabs) return;                   // (wave-uniform)
    const int32_t lane = threadIdx.x & 63;
    const uint64_t own = first + lane < n_slabs ? masks[first + lane] : 0;
    uint64_t todo = __ballot(own != 0);
    while (todo) {                                  // (wave-uniform)
        const int c = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t w = first + c;
        int32_t nb;
        const Slab s = bm_classify(set, d, thr, fill, w, lane, nb);
        const Slots8 up = bm_slots8(nb, 1), down = bm_slots8(nb, -1);
        const int32_t li = (int32_t)(w & 7), lj = lane >> 3, lk = lane & 7;
        const int32_t gi = 8 * s.cx + li, gj = 8 * s.cy + lj, gk = 8 * s.cz + lk;
        const uint64_t packed = ranks[w];
        const uint64_t below = (1ull << lane) - 1;
        bool in0 = false;
        if ((s.active >> lane) & 1) {
            float v[8];                              // corner 4 dx + 2 dy + dz
#pragma unroll
            for (int o = 0; o < 8; ++o) v[o] = bm_corner(set.values, up, fill, li + ((o >> 2) & 1), lj + ((o >> 1) & 1), lk + (o & 1));
            bool in[8];
            float p[3];
            mesh_cell_vertex(v, thr, gi, gj, gk, box, in, p);
            const int64_t rank = (int64_t)(packed & 0xffffffffull) + __popcll(s.active & below);
            if (rank < vertex_capacity) {
                vertices[3 * rank + 0] = p[0];
                vertices[3 * rank + 1] = p[1];
                vertices[3 * rank + 2] = p[2];
                if (cells) cells[rank] = ((int64_t)gi * d.ny + gj) * d.nz + gk;
            }
            in0 = in[0];
        }
        int64_t quad = (int64_t)(packed >> 32) + __popcll(s.qx & below) + __popcll(s.qy & below) + __popcll(s.qz & below);
        if ((s.qx >> lane) & 1) bm_emit_quad<0>(masks, ranks, down, li, lj, lk, in0, quad++, faces, face_capacity);
        if ((s.qy >> lane) & 1) bm_emit_quad<1>(masks, ranks, down, li, lj, lk, in0, quad++, faces, face_capacity);
        if ((s.qz >> lane) & 1) bm_emit_quad<2>(masks, ranks, down, li, lj, lk, in0, quad++, faces, face_capacity);
    }
}

// ---- the checks of the entry points -------------------------------------------------------------------------------------------------------
static int bm_dims_check(const char* who, int32_t nx, int32_t ny, int32_t nz) {
    PERF_REQUIRE(nx >= PERF_BRICKMESH_EDGE && ny >= PERF_BRICKMESH_EDGE && nz >= PERF_BRICKMESH_EDGE, "%s: a lattice of %d x %d x %d cells has a dimension below 8", who,
                 (int)nx, (int)ny, (int)nz);
    PERF_REQUIRE(nx % PERF_BRICKMESH_EDGE == 0 && ny % PERF_BRICKMESH_EDGE == 0 && nz % PERF_BRICKMESH_EDGE == 0,
                 "%s: a lattice of %d x %d x %d cells has a dimension that is not a multiple of 8", who, (int)nx, (int)ny, (int)nz);
    PERF_REQUIRE(nx <= PERF_BRICKMESH_MAX_DIM && ny <= PERF_BRICKMESH_MAX_DIM && nz <= PERF_BRICKMESH_MAX_DIM, "%s: a lattice of %d x %d x %d cells has a dimension above 4096",
                 who, (int)nx, (int)ny, (int)nz);
    return PERF_OK;
}

static int bm_bricks_check(const char* who, int32_t nx, int32_t ny, int32_t nz, int32_t n_bricks) {
    const int64_t all = (int64_t)(nx / 8) * (ny / 8) * (nz / 8);
    PERF_REQUIRE(n_bricks >= 0, "%s: a negative number of bricks (%d)", who, (int)n_bricks);
    PERF_REQUIRE(n_bricks <= PERF_BRICKMESH_MAX_BRICKS, "%s: %d bricks are more than 2^21 (2^30 cells: vertex indices are int32)", who, (int)n_bricks);
    PERF_REQUIRE(n_bricks <= all, "%s: %d bricks, the lattice has %lld", who, (int)n_bricks, (long long)all);
    return PERF_OK;
}

static int bm_occ_check(const char* who, const uint8_t* binaries, int32_t occ_res) {
    PERF_REQUIRE(binaries, "%s: NULL input (binaries)", who);
    PERF_REQUIRE(occ_res >= 1 && occ_res <= 4096, "%s: an occupancy resolution of %d is outside 1 .. 4096", who, (int)occ_res);
    return PERF_OK;
}

static int bm_workspace_check(const char* who, int32_t nx, int32_t ny, int32_t nz, int32_t n_bricks, const void* workspace, int64_t workspace_bytes) {
    return workspace_check(who, perf_brickmesh_workspace_bytes(nx, ny, nz, n_bricks), workspace, workspace_bytes);
}

static int bm_levels_check(const char* who, float thr, float fill) {
    PERF_REQUIRE(thr - thr == 0.0f, "%s: the threshold is not finite", who);
    PERF_REQUIRE(fill - fill == 0.0f, "%s: the fill value is not finite", who);
    PERF_REQUIRE(fill < thr, "%s: the fill value %g must be below the threshold %g", who, (double)fill, (double)thr);
    return PERF_OK;
}

static BrickDims bm_dims(int32_t nx, int32_t ny, int32_t nz, int32_t n_bricks) { return BrickDims{nx, ny, nz, nx / 8, ny / 8, nz / 8, n_bricks}; }

}  // namespace perf

using namespace perf;

extern "C" int perf_brickmesh_version(void) { return PERF_BRICKMESH_ABI_VERSION; }

extern "C" int64_t perf_brickmesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_bricks) {
    if (bm_dims_check("perf_brickmesh_workspace_bytes", nx, ny, nz) != PERF_OK) return -1;
    if (bm_bricks_check("perf_brickmesh_workspace_bytes", nx, ny, nz, n_bricks) != PERF_OK) return -1;
    const int64_t groups = div_up((int64_t)(nx / 8) * (ny / 8) * (nz / 8), 256);
    const int64_t select = groups + scan_words(groups);
    const int64_t slabs = 8 * (int64_t)n_bricks;
    const int64_t count = n_bricks > 0 ? 3 * slabs + 2 * scan_words(slabs) + 4 : 4;
    const int64_t words = select > count ? select : count;
    return ((words + 1) & ~(int64_t)1) * (int64_t)sizeof(uint64_t);      // (a multiple of 16)
}

extern "C" int perf_brickmesh_select(const uint8_t* binaries, int32_t occ_res, int32_t nx, int32_t ny, int32_t nz, int32_t* table, int64_t* n_live_dev,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = bm_occ_check("perf_brickmesh_select", binaries, occ_res)) return rc;
    PERF_REQUIRE(table && n_live_dev, "perf_brickmesh_select: NULL output (table or n_live_dev)");
    if (int rc = bm_dims_check("perf_brickmesh_select", nx, ny, nz)) return rc;
    if (int rc = bm_workspace_check("perf_brickmesh_select", nx, ny, nz, 0, workspace, workspace_bytes)) return rc;
    const BrickDims d = bm_dims(nx, ny, nz, 0);
    const int64_t all = (int64_t)d.bx * d.by * d.bz, groups = div_up(all, 256);
    uint64_t* sums = (uint64_t*)workspace;
    hipLaunchKernelGGL(brickmesh_select_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), binaries, occ_res, d, all, table, sums);
    const uint64_t* total = scan_u64(sums, groups, sums + groups, as_stream(stream));
    hipLaunchKernelGGL(brickmesh_select_add_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), table, all, (const uint64_t*)sums, total, n_live_dev);
    PERF_LAUNCH_CHECK("perf_brickmesh_select");
    return PERF_OK;
}

extern "C" int perf_brickmesh_list(const int32_t* table, int32_t nx, int32_t ny, int32_t nz, int32_t* ids, int32_t n_bricks, void* stream) {
    PERF_REQUIRE(table, "perf_brickmesh_list: NULL input (table)");
    if (int rc = bm_dims_check("perf_brickmesh_list", nx, ny, nz)) return rc;
    if (int rc = bm_bricks_check("perf_brickmesh_list", nx, ny, nz, n_bricks)) return rc;
    PERF_REQUIRE(ids || n_bricks == 0, "perf_brickmesh_list: NULL output (ids) with bricks to list");
    if (n_bricks == 0) return PERF_OK;
    const int64_t all = (int64_t)(nx / 8) * (ny / 8) * (nz / 8);
    hipLaunchKernelGGL(brickmesh_list_kernel, dim3((unsigned)div_up(all, 256)), dim3(256), 0, as_stream(stream), table, all, ids, n_bricks);
    PERF_LAUNCH_CHECK("perf_brickmesh_list");
    return PERF_OK;
}

extern "C" int perf_brickmesh_corners(const int32_t* ids, int32_t n_bricks, int32_t first, int32_t m, int32_t nx, int32_t ny, int32_t nz,
                                      const uint8_t* binaries, int32_t occ_res, float* x01, uint8_t* sel, uint8_t* interior, void* stream) {
    if (int rc = bm_occ_check("perf_brickmesh_corners", binaries, occ_res)) return rc;
    if (int rc = bm_dims_check("perf_brickmesh_corners", nx, ny, nz)) return rc;
    if (int rc = bm_bricks_check("perf_brickmesh_corners", nx, ny, nz, n_bricks)) return rc;
    PERF_REQUIRE(first >= 0 && m >= 0 && (int64_t)first + m <= n_bricks, "perf_brickmesh_corners: the slots %d .. %d + %d are not within the %d bricks", (int)first,
                 (int)first, (int)m, (int)n_bricks);
    if (m == 0) return PERF_OK;
    PERF_REQUIRE(ids, "perf_brickmesh_corners: NULL input (ids)");
    PERF_REQUIRE(x01 && sel, "perf_brickmesh_corners: NULL output (x01 or sel)");
    const int64_t n_corners = (int64_t)m * 512;
    hipLaunchKernelGGL(brickmesh_corners_kernel, dim3((unsigned)div_up(n_corners, 256)), dim3(256), 0, as_stream(stream), ids, first, n_corners, bm_dims(nx, ny, nz, n_bricks),
                       (int64_t)(nx / 8) * (ny / 8) * (nz / 8), binaries, occ_res, x01, sel, interior);
    PERF_LAUNCH_CHECK("perf_brickmesh_corners");
    return PERF_OK;
}

extern "C" int perf_brickmesh_count(const float* values, const int32_t* ids, const int32_t* table, int32_t n_bricks, int32_t nx, int32_t ny, int32_t nz,
                                    float thr, float fill, void* workspace, int64_t workspace_bytes, int64_t* counts_dev, void* stream) {
    PERF_REQUIRE(table, "perf_brickmesh_count: NULL input (table)");
    PERF_REQUIRE(counts_dev, "perf_brickmesh_count: NULL output (counts_dev)");
    if (int rc = bm_dims_check("perf_brickmesh_count", nx, ny, nz)) return rc;
    if (int rc = bm_bricks_check("perf_brickmesh_count", nx, ny, nz, n_bricks)) return rc;
    PERF_REQUIRE((values && ids) || n_bricks == 0, "perf_brickmesh_count: NULL input (values or ids) with bricks to mesh");
    if (int rc = bm_levels_check("perf_brickmesh_count", thr, fill)) return rc;
    if (int rc = bm_workspace_check("perf_brickmesh_count", nx, ny, nz, n_bricks, workspace, workspace_bytes)) return rc;
    const BrickDims d = bm_dims(nx, ny, nz, n_bricks);
    const BrickSet set{values, ids, table};
    const int64_t slabs = 8 * (int64_t)n_bricks;
    uint64_t* masks = (uint64_t*)workspace;
    uint64_t* ranks = masks + slabs;
    uint64_t* violations = ranks + slabs;
    uint64_t* level = violations + slabs;
    const int64_t level_words = n_bricks > 0 ? scan_words(slabs) : 0;
    int64_t* totals = (int64_t*)(level + 2 * level_words);
    const uint64_t *packed_total = nullptr, *violation_total = nullptr;
    if (n_bricks > 0) {
        hipLaunchKernelGGL(brickmesh_count_kernel, dim3((unsigned)div_up(slabs, 4)), dim3(256), 0, as_stream(stream), set, d, thr, fill, slabs, masks, ranks,
                           violations);
        packed_total = scan_u64(ranks, slabs, level, as_stream(stream));
        violation_total = scan_u64(violations, slabs, level + level_words, as_stream(stream));
    }
    hipLaunchKernelGGL(brickmesh_totals_kernel, dim3(1), dim3(64), 0, as_stream(stream), packed_total, violation_total, totals, counts_dev);
    PERF_LAUNCH_CHECK("perf_brickmesh_count");
    return PERF_OK;
}

extern "C" int perf_brickmesh_write(const float* values, const int32_t* ids, const int32_t* table, int32_t n_bricks, int32_t nx, int32_t ny, int32_t nz,
                                    float thr, float fill, const float* lo, const float* hi, const void* workspace, int64_t workspace_bytes,
                                    float* vertices, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity, int64_t* cells, void* stream) {
    PERF_REQUIRE(table && lo && hi, "perf_brickmesh_write: NULL input (table, lo or hi)");
    PERF_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, "perf_brickmesh_write: negative capacity");
    PERF_REQUIRE((vertices || vertex_capacity == 0) && (faces || face_capacity == 0), "perf_brickmesh_write: NULL output with a capacity above 0");
    if (int rc = bm_dims_check("perf_brickmesh_write", nx, ny, nz)) return rc;
    if (int rc = bm_bricks_check("perf_brickmesh_write", nx, ny, nz, n_bricks)) return rc;
    PERF_REQUIRE((values && ids) || n_bricks == 0, "perf_brickmesh_write: NULL input (values or ids) with bricks to mesh");
    if (int rc = bm_levels_check("perf_brickmesh_write", thr, fill)) return rc;
    for (int a = 0; a < 3; ++a)
        PERF_REQUIRE(hi[a] > lo[a] && hi[a] - hi[a] == 0.0f && lo[a] - lo[a] == 0.0f, "perf_brickmesh_write: the box needs finite hi > lo on every axis (axis %d: lo %g, hi %g)", a,
                     (double)lo[a], (double)hi[a]);
    if (int rc = bm_workspace_check("perf_brickmesh_write", nx, ny, nz, n_bricks, workspace, workspace_bytes)) return rc;
    const BrickDims d = bm_dims(nx, ny, nz, n_bricks);
    const BrickSet set{values, ids, table};
    const int64_t slabs = 8 * (int64_t)n_bricks;
    const uint64_t* masks = (const uint64_t*)workspace;
    const uint64_t* ranks = masks + slabs;
    const int64_t level_words = n_bricks > 0 ? scan_words(slabs) : 0;
    const int64_t* totals_dev = (const int64_t*)(ranks + 2 * slabs + 2 * level_words);
    int64_t totals[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(totals, totals_dev, sizeof(totals), hipMemcpyDeviceToHost, as_stream(stream)) != hipSuccess ||
        hipStreamSynchronize(as_stream(stream)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_brickmesh_write: reading the counted totals back failed");
        return PERF_E_LAUNCH;
    }
    PERF_REQUIRE(vertex_capacity >= totals[0], "perf_brickmesh_write: room for %lld vertices, %lld were counted", (long long)vertex_capacity, (long long)totals[0]);
    PERF_REQUIRE(face_capacity >= totals[1], "perf_brickmesh_write: room for %lld faces, %lld were counted", (long long)face_capacity, (long long)totals[1]);
    if (totals[0] == 0) return PERF_OK;              // (no active cell: no quad either)
    MeshBox box;
    const int32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = (double)lo[a];
        box.scale[a] = ((double)hi[a] - (double)lo[a]) / (double)n[a];
    }
    hipLaunchKernelGGL(brickmesh_write_kernel, dim3((unsigned)div_up(slabs, 256)), dim3(256), 0, as_stream(stream), set, d, thr, fill, box, slabs, masks, ranks,
                       vertices, vertex_capacity, faces, face_capacity, cells);
    PERF_LAUNCH_CHECK("perf_brickmesh_write");
    return PERF_OK;
}
