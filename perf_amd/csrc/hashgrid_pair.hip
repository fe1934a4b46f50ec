// Pair table (include/perf_hip_pair.h): two fields whose hash grids have the same geometry, evaluated at the same positions.
//
// The forward encode (hashgrid_fwd.hip) is paced by L1 misses in flight, not by requests or bytes, and a lane request costs the L1 the
// same at 4, 8 and 16 bytes.  Two fields at the same positions take every miss twice, at the same index in two tables.  Here the two
// tables are interleaved entry by entry -- one 8-byte word {field A, field B} -- and one gather per corner serves both fields; corner
// indices, weights and the run de-duplication are formed once.  Interpolation is per field in hashgrid_fwd_v2_kernel's order, so each
// feature array is bit-identical to the single encode's.
//
// What hashgrid_fwd2_kernel (two separate tables, 2x slower than two passes) got wrong is the resident set: an XCD's L2 holds 4 MiB and a
// hashed level of a pair table is 2 MiB at T = 2^18, so the {g, 15 - g} level groups of the single encode would put two hashed levels
// (4 MiB) on half the XCDs.  The levels are regrouped into SLOTS of at most one hashed level (plus, optionally, one dense coarse level),
// and the slots are served in PARTS of the launch, one after the other; within a part XCD x serves slot (x + phase) % slots, with the
// rotation over phases of the single encode.  Placement is a speed assumption only: results do not depend on it.
#include "common.hpp"
#include "grid_device.hpp"
#include "../../include/perf_hip_pair.h"

namespace perf {

constexpr int kPairMaxParts = 4;
constexpr int64_t kPairMaxChunks = 4096;       // chunks of 256 samples per part of one launch; the workgroups loop beyond (hashgrid_fwd.hip: kFwdMaxChunks)
constexpr int kPairShareMaxHeads = 56;         // (hashgrid_fwd.hip: kShareMaxHeads)

// parts of a launch: part p has 1 << shift[p] slots (1, 2, 4 or 8), slot s encodes level[p][s][0] and level[p][s][1] (-1: none)
struct PairPlan {
    int32_t n_parts;
    int32_t shift[kPairMaxParts];
    int32_t level[kPairMaxParts][8][2];
};

template <typename T16>
__global__ __launch_bounds__(256) void hashgrid_fwd_pair_kernel(GridParams gp, PairPlan plan, const float* __restrict__ x01,
                                                                const uint2* __restrict__ pair, uint32_t* __restrict__ feat_a,
                                                                uint32_t* __restrict__ feat_b, int64_t n,
                                                                const int64_t* __restrict__ n_dev, int64_t nchunks_grid) {
    const int64_t n_live = live_count(n, n_dev);                 // (n stays the level stride)
    const int64_t nchunks_live = (n_live + 255) >> 8;
    // the part of this workgroup (nchunks_grid is a multiple of 8: every part starts at a multiple of 8 workgroups)
    int part = 0;
    int64_t b = blockIdx.x;
    while (part + 1 < plan.n_parts && b >= (nchunks_grid << plan.shift[part])) { b -= nchunks_grid << plan.shift[part]; ++part; }
    const int sh = plan.shift[part], slots = 1 << sh;
    const int xcd = (int)(blockIdx.x & 7);
    const bool smooth = gp.interpolation == PERF_INTERP_SMOOTHSTEP;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (lane == 63u) ? ~0ull : ((2ull << lane) - 1ull);      // lanes <= mine
    // eight consecutive workgroups (one per XCD) serve 8 / slots chunks, every slot of each; chunk-stride loop as in hashgrid_fwd_v2_kernel
    for (int64_t chunk = (b >> 3) * (8 >> sh) + (xcd >> sh); chunk < nchunks_live; chunk += nchunks_grid) {
        const int64_t in_pass = chunk % nchunks_grid, pass_len = nchunks_live < nchunks_grid ? nchunks_live : nchunks_grid;
        const int phase = (int)((in_pass * slots) / pass_len);
        const int slot = (xcd + phase) & (slots - 1);
        const int64_t i = chunk * 256 + threadIdx.x;
        const bool live = i < n_live;
        const int64_t ii = live ? i : n_live - 1;                // (idle lanes of the last chunk repeat its last sample)
        int lv[2];
        lv[0] = plan.level[part][slot][0]; lv[1] = plan.level[part][slot][1];
        if (lv[0] < 0 && lv[1] < 0) continue;                    // (a padding slot)
        const float x = x01[3 * ii], y = x01[3 * ii + 1], z = x01[3 * ii + 2];
        // one level at a time, the loop kept rolled: corners, run-sharing state and the eight words of ONE level are live at once, which
        // is what holds the kernel to 64 VGPRs (eight waves per SIMD); the joint two-level body took 114 (four)
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const int l = lv[pass];
            if (l < 0) continue;
            const Corners c = corners_of(x, y, z, gp.scale[l], gp.res[l], gp.size[l], gp.hashed[l] != 0);
            // lane - 1's cell through DPP (wave_shr:1; lane 0 keeps the `old` operand)
            const uint32_t px = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)c.cell[0], 0x138, 0xf, 0xf, false);
            const uint32_t py = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)c.cell[1], 0x138, 0xf, 0xf, false);
            const uint32_t pz = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)c.cell[2], 0x138, 0xf, 0xf, false);
            const bool same = lane != 0u && px == c.cell[0] && py == c.cell[1] && pz == c.cell[2];
            const unsigned long long heads = __ballot(!same);
            const bool share = __popcll(heads) <= kPairShareMaxHeads;      // wave-uniform
            const bool head = share ? !same : true;
            const uint32_t src = share ? 63u - (uint32_t)__clzll((long long)(heads & below)) : lane;     // the head of my run
            uint2 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = make_uint2(0u, 0u);
            if (head) {
                const uint2* t = pair + gp.offset[l];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = t[c.idx[k]];
            }
            if (share) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    v[k].x = (uint32_t)__shfl((int)v[k].x, (int)src);
                    v[k].y = (uint32_t)__shfl((int)v[k].y, (int)src);
                }
            }
            float w[8];
            corner_weights(c.f, smooth, w);
            float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a0 = fmaf(w[k], T16::lo(v[k].x), a0);
                a1 = fmaf(w[k], T16::hi(v[k].x), a1);
                b0 = fmaf(w[k], T16::lo(v[k].y), b0);
                b1 = fmaf(w[k], T16::hi(v[k].y), b1);
            }
            if (live) {
                const int64_t o = (int64_t)l * n + i;
                feat_a[o] = T16::pack(a0, a1);
                feat_b[o] = T16::pack(b0, b1);
            }
        }
    }
}

__global__ __launch_bounds__(256) void pair_fill_kernel(uint32_t* __restrict__ pair, int field, const uint32_t* __restrict__ table,
                                                        int64_t n_entries) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_entries; e += (int64_t)gridDim.x * 256)
        pair[2 * e + field] = table[e];
}

// The slots of a grid: every hashed level alone, then the dense (coarse, small) levels, each beside one of the finest hashed levels -- no
// XCD ever gathers from more than one hashed level.  Measured on 8192 x 128 ray-ordered samples, bf16, L16 / T18, against 0.334 ms for two
// single encodes (tools/exp/pair_encode.py, profiles/pair_encode.json): this grouping 0.218 ms; every level alone in two halves of eight
// 0.235; the single encode's {g, 15 - g} (two hashed levels, 4 MiB, on half the XCDs) 0.234 -- on uniform points 0.382, where this grouping
// takes 0.321; non-temporal feature stores change nothing (0.218).  The retired switches: tools/exp/pair_encode_variants.diff.
// Measured again with the level-at-a-time body at eight waves per SIMD (profiles/pair_levels.json): this grouping 0.205, every level alone
// 0.221 (uniform points 0.322 either way); held to five waves 0.207, two samples per thread 0.223: tools/exp/pair_levels_variants.diff.
static void pair_plan(const GridParams& gp, PairPlan* plan) {
    int slot[16][2], n_slots = 0;
    const int L = gp.n_levels;
    int n_dense = 0, n_hashed = 0, dense[16], hashed[16];
    for (int l = 0; l < L; ++l) { if (gp.hashed[l]) hashed[n_hashed++] = l; else dense[n_dense++] = l; }
    const int n_both = n_dense < n_hashed ? n_dense : n_hashed;
    for (int k = 0; k < n_hashed - n_both; ++k) { slot[n_slots][0] = hashed[k]; slot[n_slots][1] = -1; ++n_slots; }
    for (int k = 0; k < n_dense; ++k) { slot[n_slots][0] = dense[k]; slot[n_slots][1] = k < n_both ? hashed[n_hashed - 1 - k] : -1; ++n_slots; }
    plan->n_parts = 0;
    for (int p = 0; p < kPairMaxParts; ++p) {
        plan->shift[p] = 0;
        for (int s = 0; s < 8; ++s) plan->level[p][s][0] = plan->level[p][s][1] = -1;
    }
    for (int s0 = 0; s0 < n_slots; s0 += 8) {
        const int p = plan->n_parts++, left = n_slots - s0 < 8 ? n_slots - s0 : 8;
        int sh = 0;
        while ((1 << sh) < left) ++sh;                            // (a part of 3, 5, 6 or 7 slots is padded with empty ones)
        plan->shift[p] = sh;
        for (int s = 0; s < left; ++s) { plan->level[p][s][0] = slot[s0 + s][0]; plan->level[p][s][1] = slot[s0 + s][1]; }
    }
}

}  // namespace perf

using namespace perf;

extern "C" int perf_pair_version(void) { return PERF_PAIR_ABI_VERSION; }

extern "C" int perf_pair_fill(void* pair, int field, const void* table16, int64_t n_entries, void* stream) {
    PERF_REQUIRE(n_entries >= 0 && n_entries < (int64_t(1) << 40), "perf_pair_fill: n_entries out of range");
    PERF_REQUIRE(field == 0 || field == 1, "perf_pair_fill: field %d is neither 0 nor 1", field);
    if (n_entries == 0) return PERF_OK;
    PERF_REQUIRE(pair && table16, "perf_pair_fill: NULL pointer");
    PERF_REQUIRE(((uintptr_t)pair & 7u) == 0 && ((uintptr_t)table16 & 3u) == 0, "perf_pair_fill: the pair table must be 8-byte, the table 4-byte aligned");
    int64_t blocks = div_up(n_entries, 256);
    if (blocks > 8 * kNumCU) blocks = 8 * kNumCU;
    hipLaunchKernelGGL(pair_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (uint32_t*)pair, field, (const uint32_t*)table16, n_entries);
    PERF_LAUNCH_CHECK("perf_pair_fill");
    return PERF_OK;
}

extern "C" int perf_hashgrid_fwd_pair(const perf_grid_desc* grid, const float* x01, const void* pair, void* feat16_a, void* feat16_b,
                                      int64_t n, const int64_t* n_dev, int dtype, void* stream) {
    GridParams gp;
    int rc = fill_params(grid, &gp);                              // (refuses line-local layouts)
    if (rc) return rc;
    PERF_REQUIRE(gp.n_levels <= 16, "perf_hashgrid_fwd_pair: %d levels (built for at most 16)", gp.n_levels);
    PERF_REQUIRE(n >= 0 && n < (int64_t(1) << 31) * 16, "perf_hashgrid_fwd_pair: n out of range");
    PERF_REQUIRE(dtype == PERF_DTYPE_BF16 || dtype == PERF_DTYPE_FP16, "perf_hashgrid_fwd_pair: bad dtype %d", dtype);
    if (n == 0) return PERF_OK;
    PERF_REQUIRE(x01 && pair && feat16_a && feat16_b, "perf_hashgrid_fwd_pair: NULL pointer");
    PERF_REQUIRE(((uintptr_t)pair & 7u) == 0, "perf_hashgrid_fwd_pair: the pair table must be 8-byte aligned");
    PairPlan plan;
    pair_plan(gp, &plan);
    int64_t chunks = div_up(div_up(n, 256), 8) * 8;
    if (chunks > kPairMaxChunks) chunks = kPairMaxChunks;
    int64_t blocks = 0;
    for (int p = 0; p < plan.n_parts; ++p) blocks += chunks << plan.shift[p];
    dim3 g((unsigned)blocks), b(256);
    if (dtype == PERF_DTYPE_BF16)
        hipLaunchKernelGGL(hashgrid_fwd_pair_kernel<BF16>, g, b, 0, as_stream(stream), gp, plan, x01, (const uint2*)pair, (uint32_t*)feat16_a, (uint32_t*)feat16_b, n, n_dev, chunks);
    else
        hipLaunchKernelGGL(hashgrid_fwd_pair_kernel<FP16>, g, b, 0, as_stream(stream), gp, plan, x01, (const uint2*)pair, (uint32_t*)feat16_a, (uint32_t*)feat16_b, n, n_dev, chunks);
    PERF_LAUNCH_CHECK("perf_hashgrid_fwd_pair");
    return PERF_OK;
}
