// Step riders (include/perf_hip_riders.h): the front end of the next training batch as workgroups of 256 threads that ride in launches
// of the current step's backward.  Each stage calls the device function its stand-alone kernel calls -- one body, the same bits.
#pragma once
#include "common.hpp"
#include "march_device.hpp"
#include "../../include/perf_hip_riders.h"

namespace perf {

// ---- the batch draw (misc.hip: perf_gather_supervision, perf_draw_train_batch) ----------------------------------------------------
// The rows of pixel j -> slot i of whatever outputs are asked for.  ALL the loads are issued before the first store: written as
// "if (o) o[..] = o_all[..]" per element, every load is waited for on its own before the store that follows it -- thirteen
// dependent round trips to random rows for what is one (11 us -> the latency of one gather, measured on the draw kernel).
__device__ __forceinline__ void gather_rows(int64_t i, int64_t j, const float* __restrict__ o_all, const float* __restrict__ d_all,
                                            const float* __restrict__ c_all, const float* __restrict__ t_all,
                                            const float* __restrict__ n_all, float* __restrict__ o, float* __restrict__ d,
                                            float* __restrict__ c, float* __restrict__ t, float* __restrict__ nrm) {
    float vo[3] = {0.f, 0.f, 0.f}, vd[3] = {0.f, 0.f, 0.f}, vc[3] = {0.f, 0.f, 0.f}, vn[3] = {0.f, 0.f, 0.f}, vt = 0.f;
    if (o) { vo[0] = o_all[3 * j]; vo[1] = o_all[3 * j + 1]; vo[2] = o_all[3 * j + 2]; }
    if (d) { vd[0] = d_all[3 * j]; vd[1] = d_all[3 * j + 1]; vd[2] = d_all[3 * j + 2]; }
    if (c) { vc[0] = c_all[3 * j]; vc[1] = c_all[3 * j + 1]; vc[2] = c_all[3 * j + 2]; }
    if (nrm) { vn[0] = n_all[3 * j]; vn[1] = n_all[3 * j + 1]; vn[2] = n_all[3 * j + 2]; }
    if (t) vt = t_all[j];
    if (o) { o[3 * i] = vo[0]; o[3 * i + 1] = vo[1]; o[3 * i + 2] = vo[2]; }
    if (d) { d[3 * i] = vd[0]; d[3 * i + 1] = vd[1]; d[3 * i + 2] = vd[2]; }
    if (c) { c[3 * i] = vc[0]; c[3 * i + 1] = vc[1]; c[3 * i + 2] = vc[2]; }
    if (nrm) { nrm[3 * i] = vn[0]; nrm[3 * i + 1] = vn[1]; nrm[3 * i + 2] = vn[2]; }
    if (t) t[i] = vt;
}

// Philox4x32-10 (Salmon et al., SC'11; the counter-based generator family torch.rand uses on the GPU): 128-bit counter,
// 64-bit key -> four 32-bit words.
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x & 0xffffffu) * (1.0f / 16777216.0f); }   // 24 bits, [0, 1)

// Workgroup `block` of the `n_blocks` (256 threads each) that draw a batch -- draw_train_batch_kernel is this body.
__device__ __forceinline__ void draw_train_batch_body(int block, int n_blocks, uint32_t seed_lo, uint32_t seed_hi, int64_t* __restrict__ counter,
                                                      int32_t* __restrict__ ticket, int64_t pool_lo, int64_t pool_n,
                                                      int64_t n_local, int64_t first_global,
                                                      const float* __restrict__ o_all, const float* __restrict__ d_all,
                                                      const float* __restrict__ c_all, const float* __restrict__ t_all,
                                                      const float* __restrict__ n_all, float* __restrict__ o,
                                                      float* __restrict__ d, float* __restrict__ c, float* __restrict__ t,
                                                      float* __restrict__ nrm, int64_t* __restrict__ idx_out,
                                                      float* __restrict__ jitter, float* __restrict__ noise,
                                                      float* __restrict__ bg) {
    const uint64_t draw = (uint64_t)counter[0];              // read by every workgroup BEFORE any of them can advance it
    const int64_t i = (int64_t)block * 256 + threadIdx.x;
    if (i < n_local) {
        const uint64_t g = (uint64_t)(first_global + i);     // position in the GLOBAL batch: ranks draw disjoint slices of one stream
        uint32_t r[4] = {(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)draw, (uint32_t)(draw >> 32) & 0x7fffffffu};
        philox4x32_10(r, seed_lo, seed_hi);
        const int64_t j = pool_lo + (int64_t)(((uint64_t)r[0] * (uint64_t)pool_n) >> 32);
        gather_rows(i, j, o_all, d_all, c_all, t_all, n_all, o, d, c, t, nrm);     // (first: its loads fly during the second Philox)
        if (idx_out) idx_out[i] = j;
        if (jitter) jitter[i] = u01(r[1]);
        if (noise) noise[i] = u01(r[2]);
        if (bg) {
            uint32_t q[4] = {(uint32_t)g, (uint32_t)(g >> 32), (uint32_t)draw, ((uint32_t)(draw >> 32) & 0x7fffffffu) | 0x80000000u};
            philox4x32_10(q, seed_lo, seed_hi);
            bg[3 * i] = u01(q[0]); bg[3 * i + 1] = u01(q[1]); bg[3 * i + 2] = u01(q[2]);
        }
    }
    // the last workgroup to finish advances the draw counter (every workgroup has read it by then) and rearms the ticket
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(ticket, 1) == n_blocks - 1) {
        counter[0] = (int64_t)(draw + 1);
        *ticket = 0;
    }
}

// ---- the jobs as the kernels receive them: the header's argument blocks plus what the host derives once --------------------------------
// n_blocks == 0: no rider, the host launch is exactly what it is without one.
struct RiderDrawJob {        // stage A
    perf_rider_draw a;
    int32_t k_need;          // lattice indices a table of runs must reach
    int32_t n_blocks;        // ceil(n_local / PERF_RIDER_DRAW_RAYS)
};
struct RiderCountJob {       // stage B
    MarchParams mp;
    const float *ro, *rd, *t0s;
    float t0_scale, t0_base;
    int64_t n_rays;
    const uint32_t *bits, *coarse;
    const int32_t* runs;
    uint64_t* masks;
    int32_t* counts;
    int32_t n_blocks;        // ceil(n_rays / PERF_RIDER_MARCH_RAYS)
};
struct RiderWriteJob {       // stage C
    perf_rider_write a;
    Aabb bb;
    int32_t mask_words;
    int32_t n_blocks;        // ceil(n_rays / PERF_RIDER_MARCH_RAYS)
};

__device__ __forceinline__ void rider_draw_block(const RiderDrawJob& j, int block) {
    const perf_rider_draw& a = j.a;
    if (a.marched_keep && block == 0 && threadIdx.x == 0) a.marched_keep[0] = a.marched_live[0];
    draw_train_batch_body(block, j.n_blocks, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.counter_dev, a.ticket, a.pool_lo, a.pool_hi - a.pool_lo,
                          a.n_local, a.first_global, a.o_all, a.d_all, a.color_all, a.dist_all, a.normal_all, a.o, a.d, a.color, a.dist, a.normal,
                          a.indices_out, a.jitter, a.noise, a.bg);
    // (the lane reads back the draw it stored itself, behind the body's barrier)
    lattice_runs_row((int64_t)block * PERF_RIDER_DRAW_RAYS + threadIdx.x, a.jitter, a.t0_scale, a.t0_base, a.n_local, a.step, j.k_need, a.runs);
}

__device__ __forceinline__ void rider_count_block(const RiderCountJob& j, int block) {
    SharedRuns none;         // (per-ray origins: no table shared by the launch)
    none.n = 0;
    march_count_body<false>(block, j.mp, j.ro, j.rd, j.t0s, j.n_rays, j.bits, j.coarse, j.masks, j.counts, HeadOut{}, j.t0_scale, j.t0_base, none,
                            reinterpret_cast<const float*>(j.runs));
}

// The offsets of the workgroup's four rays are the sum of the counts before them, added up here (coalesced 16-byte loads of at most
// 4 PERF_RIDER_MAX_RAYS bytes from L2, as scan_small_kernel does for its segment) -- no scan launch; then the write pass.
__device__ __forceinline__ void rider_write_block(const RiderWriteJob& j, int block) {
    const perf_rider_write& a = j.a;
    __shared__ long long before4[4];
    long long s = 0;
    const int4* c4 = reinterpret_cast<const int4*>(a.counts);          // (16-byte aligned: checked on the host)
    for (int i = threadIdx.x; i < block; i += PERF_RIDER_THREADS) { const int4 v = c4[i]; s += (long long)v.x + v.y + v.z + v.w; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) before4[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = (before4[0] + before4[1]) + (before4[2] + before4[3]);
        const int64_t r0 = (int64_t)block * PERF_RIDER_MARCH_RAYS;
        for (int k = 0; k < PERF_RIDER_MARCH_RAYS; ++k)
            if (r0 + k < a.n_rays) { a.offsets[r0 + k] = (int32_t)run; run += a.counts[r0 + k]; }
        if (r0 + PERF_RIDER_MARCH_RAYS >= a.n_rays) a.total[0] = run;
    }
    __syncthreads();         // (the four offsets: written by this workgroup, read by this workgroup)
    SharedRuns none;
    none.n = 0;
    march_write_body(block, j.n_blocks, a.t0, a.n_rays, a.step, j.mask_words, a.masks, a.counts, a.offsets, a.capacity, a.ray_indices, a.t_starts,
                     a.t_ends, a.packed_info, a.rays_o, a.rays_d, j.bb, a.x01, a.sel, 0, a.t0_scale, a.t0_base, PERF_LATTICE_REPEATED, none,
                     reinterpret_cast<const float*>(a.runs));
}

}  // namespace perf

// the host side of the jobs (march.hip; hidden: not part of the C ABI): argument checks and derived fields; n_blocks = 0 for a NULL
// argument block
#define PERF_INTERNAL_RIDERS __attribute__((visibility("hidden")))
PERF_INTERNAL_RIDERS int perf_internal_rider_draw_job(const perf_rider_draw* a, perf::RiderDrawJob* job);
PERF_INTERNAL_RIDERS int perf_internal_rider_count_job(const perf_rider_count* a, perf::RiderCountJob* job);
PERF_INTERNAL_RIDERS int perf_internal_rider_write_job(const perf_rider_write* a, perf::RiderWriteJob* job);
