// Hash-grid parameter gradient of the line-local table layouts (PERF_LAYOUT_LINE_LOCAL / _OVERLAP, include/perf_hip.h) for gfx950.
//
// A grid of either layout is a PREFIX of levels under tcnn's rule (res < local_min_res) followed by a SUFFIX of line-local levels (res
// grows with the level).  The prefix goes through perf_internal_hashgrid_bwd unchanged, on a descriptor that holds only those levels
// (same offsets, same dfeat rows).  The suffix gets the owners of this unit: one 1,024-thread workgroup per (level, tile, replica) keeps
// 16,384 consecutive entries of the level in LDS -- fp32 pairs or the packed 64-bit fixed-point fields of hashgrid_bwd.hip, in the
// same units (fixed_point_shift) -- streams every sample of its level, and applies the corners that fall in its tile.  A corner of
// entry idx belongs to tile idx >> 14 whatever the super-block shape: a line-local level starts on a super-block boundary, so a
// super-block of at most 2^14 entries lies in one tile and a larger one is cut into slabs of 512 consecutive 4 x 4 x 2 blocks.
// Corner indices come from the forward's own addressing (corners_of_any).  Levels of more than 255 tiles, and workspaces without
// room for the owners' replica slabs, take a global-atomics scatter with the same weight association and units: in fixed-point
// mode both paths add the same integers, so the tables are bit-identical.
//
// LINE_OVERLAP: position 3 of x run k and position 0 of run k + 1 of a super-block row hold ONE vertex.  Both entries receive the
// sum of the two contributions (the owners fold them in LDS before the write-back; the scatter adds a shared vertex's update into
// both copies), and the never-read last entry of a row's last run receives 0.  Adam being elementwise, the two copies of every
// shared vertex then stay bit-equal through training.
#include <mutex>
#include "common.hpp"
#include "grid_device.hpp"
#include "grid_fixed_point.hpp"
#include "mlp_reduce_device.hpp"
#include "step_book_device.hpp"

namespace perf {

constexpr int kLnTileShift = 14;
constexpr uint32_t kLnTileEntries = 1u << kLnTileShift;
constexpr int kLnThreads = 1024;
constexpr int kLnMaxTiles = 255;            // owners per level at most (beyond: the global-atomics scatter)
constexpr int kLnCus = 248;                 // (hashgrid_bwd.hip kCus: what a launch of 128 KiB owners is given at most)
constexpr int kLnMaxReplicas = 8;

struct LinesPlan {
    uint32_t owner_levels;                  // bit l: line-local level on LDS owners
    uint32_t atomic_levels;                 // bit l: line-local level on the global-atomics scatter
    int32_t first_block[PERF_MAX_LEVELS];   // first workgroup of the level's owners
    int32_t tiles_of[PERF_MAX_LEVELS];
    int32_t replicas_of[PERF_MAX_LEVELS];
    int64_t ws_off[PERF_MAX_LEVELS];        // float2 offset of the level's replica slabs
    int32_t n_blocks;
    int32_t accumulate;
    int32_t code_slot[PERF_MAX_LEVELS];     // >= 0: the level's tile codes are codes[slot][n_pad] (hashgrid_bwd_lines_codes_kernel)
    int64_t n_pad;
};

// Owners for levels of <= 255 tiles.  Levels of few tiles are replicated (each replica streams 1 / R of the samples into a slab of its
// own, summed by hashgrid_bwd_lines_reduce_kernel) while the launch still fits one workgroup per CU: an owner's cost is the stream of
// its level's samples plus the updates that hit it, and a one-tile level takes all eight updates of every sample.
static void plan_lines(const GridParams& gp, const GridLocal& gl, bool owners, bool replicas, LinesPlan* lp, int64_t* slab_entries) {
    lp->owner_levels = lp->atomic_levels = 0u;
    lp->n_blocks = 0; lp->accumulate = 0; lp->n_pad = 0;
    for (int l = 0; l < PERF_MAX_LEVELS; ++l) lp->code_slot[l] = -1;
    int64_t ws = 0;
    for (int l = 0; l < PERF_MAX_LEVELS; ++l) { lp->first_block[l] = 0; lp->tiles_of[l] = 0; lp->replicas_of[l] = 1; lp->ws_off[l] = 0; }
    int nb = 0;
    for (int l = 0; l < gp.n_levels; ++l) {
        if (!gl.local[l]) continue;
        const int nt = (int)((gp.size[l] + kLnTileEntries - 1u) >> kLnTileShift);
        if (!owners || nt > kLnMaxTiles) { lp->atomic_levels |= 1u << l; continue; }
        lp->owner_levels |= 1u << l;
        lp->tiles_of[l] = nt;
        nb += nt;
    }
    if (replicas) {
        for (int want = kLnMaxReplicas; want >= 2; want /= 2)
            for (int l = 0; l < gp.n_levels; ++l) {
                if (!((lp->owner_levels >> l) & 1u)) continue;
                const int nt = lp->tiles_of[l], r = lp->replicas_of[l];
                if (nt * want > 16 || want <= r || nb + nt * (want - r) > kLnCus) continue;
                nb += nt * (want - r);
                lp->replicas_of[l] = want;
            }
    }
    nb = 0;
    for (int l = 0; l < gp.n_levels; ++l) {
        if (!((lp->owner_levels >> l) & 1u)) continue;
        lp->first_block[l] = nb;
        nb += lp->tiles_of[l] * lp->replicas_of[l];
        if (lp->replicas_of[l] > 1) { lp->ws_off[l] = ws; ws += (int64_t)lp->replicas_of[l] * gp.size[l]; }
    }
    lp->n_blocks = nb;
    *slab_entries = ws;
}

// LINE_OVERLAP: the other storage entry of the vertex held by entry idx of a line-local level (position 3 of a run <-> position 0 of the
// next run of the same super-block row: idx + 29 / idx - 29, entry = ... + (block << 5) + x % 4 with the block's x part in its low bits),
// or 0xffffffff for a vertex stored once
__device__ __forceinline__ uint32_t overlap_twin(const GridLocal& gl, uint32_t idx) {
    const uint32_t runs_m = (1u << (gl.shx - 2)) - 1u, xb = (idx >> 5) & runs_m, pos = idx & 3u;
    if (pos == 3u && xb != runs_m) return idx + 29u;
    if (pos == 0u && xb != 0u) return idx - 29u;
    return 0xffffffffu;
}

// the fixed-point word of one corner update: two signed 32-bit fields packed as hi * 2^32 + lo (hashgrid_bwd.hip's units)
__device__ __forceinline__ unsigned long long fixed_word(float w, float sx, float sy) {
    return (unsigned long long)(((long long)__float2int_rn(w * sy) << 32) + (long long)__float2int_rn(w * sx));
}

// One sample's updates of tile t of line-local level l.  one_tile_sb (sum(sb_shift) <= 14): a cell whose eight corners share a
// super-block -- no face of one crossed -- lies in ONE tile, the tile of its corner 0: that single test turns most samples away before
// the eight indices are formed.
template <bool FIXED>
__device__ __forceinline__ void line_apply(const GridParams& gp, const GridLocal& gl, int l, uint32_t t, bool one_tile_sb, bool smooth,
                                           float to_fixed, float* lds, const float2 g, float x, float y, float z) {
    const uint32_t size = gp.size[l];
    if (one_tile_sb) {
        const float s = gp.scale[l];
        const uint32_t gx = (uint32_t)(int32_t)floorf(grid_pos(x, s)), gy = (uint32_t)(int32_t)floorf(grid_pos(y, s)),
                       gz = (uint32_t)(int32_t)floorf(grid_pos(z, s));
        const uint32_t X0 = gl.ovl ? overlap_x(gx) : gx, X1 = gl.ovl ? overlap_x1(gl, X0) : gx + 1u;
        const bool inside = (X0 >> gl.shx) == (X1 >> gl.shx) && (gy >> gl.shy) == ((gy + 1u) >> gl.shy) && (gz >> gl.shz) == ((gz + 1u) >> gl.shz);
        if (inside && (local_vertex_index(gl, l, size, gp.hashed[l] != 0, X0, gy, gz) >> kLnTileShift) != t) return;
    }
    const Corners c = corners_of_any(gp, gl, l, x, y, z);
    uint32_t match = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) match |= ((c.idx[k] >> kLnTileShift) == t && c.idx[k] < size ? 1u : 0u) << k;
    if (!match) return;
    float w[8];
    corner_weights(c.f, smooth, w);
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds);
    const float sx = g.x * to_fixed, sy = g.y * to_fixed;
#pragma unroll
    for (int k = 0; k < 8; ++k) {               // (static k: the corner arrays stay in registers)
        if (!((match >> k) & 1u)) continue;
        const uint32_t a = c.idx[k] & (kLnTileEntries - 1u);
        if (FIXED) atomicAdd(&lds64[a], fixed_word(w[k], sx, sy));
        else { unsafeAtomicAdd(&lds[2 * a], w[k] * g.x); unsafeAtomicAdd(&lds[2 * a + 1], w[k] * g.y); }
    }
}

// ---- tile codes: the owners of a level all test every sample, so the eight corner indices are formed ONCE per (sample, level) by a
// pre-pass that leaves the tile of each corner as one byte of a 64-bit code (0xff: no update -- zero gradient, or an index past a dense
// level's end; a level has at most 255 tiles, 0..254).  An owner then streams 8 bytes per sample instead of 20, finds the corners that
// name its tile with a few bit operations, and keeps only those samples -- a few per cent -- in a wave-private LDS queue that is
// applied 64 at a time at full lane occupancy (hashgrid_bwd.hip's coded owners do the same with 4-byte (y, z) codes).
constexpr int kLnQueueCap = 128;            // per wave: < 64 left over + 64 new per step

__global__ __launch_bounds__(256) void hashgrid_bwd_lines_codes_kernel(GridParams gp, GridLocal gl, LinesPlan lp, const float* __restrict__ x01,
                                                                       const float2* __restrict__ dfeat, unsigned long long* __restrict__ codes,
                                                                       int64_t n, const int64_t* __restrict__ n_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int l = blockIdx.y;
    if (lp.code_slot[l] < 0 || i >= live_count(n, n_dev)) return;
    const float2 g = dfeat[(int64_t)l * n + i];
    unsigned long long code = ~0ull;
    if (!(g.x == 0.f && g.y == 0.f)) {
        const Corners c = corners_of_any(gp, gl, l, x01[3 * i], x01[3 * i + 1], x01[3 * i + 2]);
        code = 0ull;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            code |= (unsigned long long)(c.idx[k] < gp.size[l] ? (c.idx[k] >> kLnTileShift) : 0xffu) << (8 * k);
    }
    codes[(int64_t)lp.code_slot[l] * lp.n_pad + i] = code;
}

// Coded owner loop: two consecutive samples per lane and step (one 16-byte load of codes, the next step's load in flight while this
// one is tested -- a lane that waited for every 8-byte code took 0.63 ms per owner at 1 M samples), matches into the wave's queue,
// the queue drained 64 at a time.
template <bool FIXED>
__device__ __forceinline__ void line_stream_codes(const GridParams& gp, const GridLocal& gl, int l, uint32_t t, bool smooth, float to_fixed,
                                                  float* lds, uint32_t* queue, const unsigned long long* __restrict__ codes_l,
                                                  const float* __restrict__ x01, const float2* __restrict__ g_l, int64_t n_live, int rep, int R) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t qn = 0;                                    // wave-uniform queue fill
    const unsigned long long t8 = (unsigned long long)t * 0x0101010101010101ull;
    auto drain = [&]() {                                // the youngest min(qn, 64) entries
        const uint32_t take = qn < 64u ? qn : 64u;
        __builtin_amdgcn_wave_barrier();
        const bool live = lane < take;
        const uint32_t i = live ? queue[qn - take + lane] : 0u;
        __builtin_amdgcn_wave_barrier();
        qn -= take;
        if (!live) return;
        const float2 g = g_l[i];
        line_apply<FIXED>(gp, gl, l, t, false, smooth, to_fixed, lds, g, x01[3 * (size_t)i], x01[3 * (size_t)i + 1], x01[3 * (size_t)i + 2]);
    };
    // codes of samples i, i + 1 (~0: past the live count -- no byte of it is a tile); codes_l is 16-byte aligned and i even
    auto load2 = [&](int64_t i, unsigned long long& a, unsigned long long& b) {
        a = b = ~0ull;
        if (i + 1 < n_live) { const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(codes_l + i); a = v.x; b = v.y; }
        else if (i < n_live) a = codes_l[i];
    };
    auto test_enqueue = [&](unsigned long long code, uint32_t i) {
        const unsigned long long x = code ^ t8;        // a zero byte: a corner in this tile
        const bool hit = ((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull) != 0ull;
        const unsigned long long b = __ballot(hit);
        if (b) {
            const uint32_t pos = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (hit) queue[pos] = i;
            qn += (uint32_t)__popcll(b);
        }
        if (qn >= 64u) drain();                         // (the fill stays below 128 = kLnQueueCap)
    };
    const int64_t step = 2 * (int64_t)R * kLnThreads;
    const int64_t first = 2 * ((int64_t)rep * kLnThreads + (threadIdx.x & ~63u));
    unsigned long long c0, c1;
    load2(first + 2 * lane, c0, c1);
    for (int64_t base = first; base < n_live; base += step) {       // wave-uniform trip count
        unsigned long long n0, n1;
        load2(base + step + 2 * lane, n0, n1);
        const uint32_t i = (uint32_t)(base + 2 * lane);
        test_enqueue(c0, i);
        test_enqueue(c1, i + 1u);
        c0 = n0; c1 = n1;
    }
    while (qn) drain();
}

// FIXED: packed fixed-point LDS fields (units of fixed_point_shift, overflow flag and headroom feedback as in hashgrid_bwd_kernel).
// redo_flag != NULL: the predicated fp32 repair launch (perf_hashgrid_bwd's redo_flag) of the line-local levels; with book it also
// carries the step's bookkeeping (a grid without tcnn-rule levels has no other repair launch to ride in).
template <bool FIXED>
__global__ __launch_bounds__(kLnThreads) void hashgrid_bwd_lines_kernel(GridParams gp, GridLocal gl, LinesPlan lp, const float* __restrict__ x01,
                                                                        const float2* __restrict__ dfeat, float2* __restrict__ grad,
                                                                        float2* __restrict__ ws, const float* __restrict__ level_absmax,
                                                                        int32_t* __restrict__ overflow_flag, int32_t* __restrict__ hr_state, int64_t n,
                                                                        const int64_t* __restrict__ n_dev, const int32_t* __restrict__ redo_flag,
                                                                        perf_step_book book, int has_book, const unsigned long long* __restrict__ codes) {
    if constexpr (!FIXED) {
        if (redo_flag && has_book && blockIdx.x == 0 && threadIdx.x == 0) step_bookkeeping_thread(book, false);
    }
    if (redo_flag && redo_flag[0] == 0) return;
    if (redo_flag && hr_state && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&hr_state[2 * PERF_MAX_LEVELS + 1], 1);   // (statistics)
    const int64_t n_live = live_count(n, n_dev);
    extern __shared__ __attribute__((aligned(16))) float lds[];      // 2 * kLnTileEntries floats (+ the wave queues of the coded loop)
    unsigned long long* lds64 = reinterpret_cast<unsigned long long*>(lds);
    int l = 0;
    while (!((lp.owner_levels >> l) & 1u) || (int)blockIdx.x >= lp.first_block[l] + lp.tiles_of[l] * lp.replicas_of[l]) ++l;
    const int R = lp.replicas_of[l];
    const int b = (int)blockIdx.x - lp.first_block[l];
    const uint32_t t = (uint32_t)(b / R);
    const int rep = b % R;
    const uint32_t size = gp.size[l];
#ifdef PERF_BWD_BLOCK_TIMES         // tools/exp/bwd_lines_block_times.py: per-workgroup durations (hashgrid_bwd.hip has the same hook)
    const long long block_t0 = wall_clock64();
#endif
    for (int i = threadIdx.x; i < 2 * (int)kLnTileEntries / 4; i += kLnThreads) reinterpret_cast<float4*>(lds)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    float to_fixed = 1.0f, from_fixed = 1.0f;
    if (FIXED) {
        const int sh = fixed_point_shift(level_absmax[l], n_live, size, hr_state, l);
        to_fixed = ldexpf(1.0f, sh);
        from_fixed = ldexpf(1.0f, -sh);
    }
    const bool smooth = gp.interpolation == PERF_INTERP_SMOOTHSTEP;
    const bool one_tile_sb = gl.shx + gl.shy + gl.shz <= (uint32_t)kLnTileShift;
    const float2* g_l = dfeat + (int64_t)l * n;
    // ---- stream this replica's samples: 4 consecutive samples per thread and step, 3 x 16 B of positions + 2 x 16 B of gradients,
    //      the next group in flight while the current one is applied (bwd_stream's skeleton)
    const int64_t n_full = n_live / 4;
    const bool aligned = ((reinterpret_cast<uintptr_t>(x01) | reinterpret_cast<uintptr_t>(g_l)) & 15) == 0;
    auto apply = [&](float gx_, float gy_, float x, float y, float z) {
        if (!(gx_ == 0.f && gy_ == 0.f)) line_apply<FIXED>(gp, gl, l, t, one_tile_sb, smooth, to_fixed, lds, make_float2(gx_, gy_), x, y, z);
    };
    if (codes && lp.code_slot[l] >= 0) {
        uint32_t* queue = reinterpret_cast<uint32_t*>(lds + 2 * kLnTileEntries) + (threadIdx.x >> 6) * kLnQueueCap;
        line_stream_codes<FIXED>(gp, gl, l, t, smooth, to_fixed, lds, queue, codes + (int64_t)lp.code_slot[l] * lp.n_pad, x01, g_l, n_live, rep, R);
    } else if (aligned) {
        const float4* x4 = reinterpret_cast<const float4*>(x01);
        const float4* g4 = reinterpret_cast<const float4*>(g_l);
        int64_t grp = (int64_t)rep * kLnThreads + threadIdx.x;
        const int64_t gstride = (int64_t)R * kLnThreads;
        float4 xa = {}, xb = {}, xc = {}, ga = {}, gb = {};
        if (grp < n_full) { xa = x4[3 * grp]; xb = x4[3 * grp + 1]; xc = x4[3 * grp + 2]; ga = g4[2 * grp]; gb = g4[2 * grp + 1]; }
        while (grp < n_full) {
            const float4 cxa = xa, cxb = xb, cxc = xc, cga = ga, cgb = gb;
            grp += gstride;
            if (grp < n_full) { xa = x4[3 * grp]; xb = x4[3 * grp + 1]; xc = x4[3 * grp + 2]; ga = g4[2 * grp]; gb = g4[2 * grp + 1]; }
            apply(cga.x, cga.y, cxa.x, cxa.y, cxa.z);
            apply(cga.z, cga.w, cxa.w, cxb.x, cxb.y);
            apply(cgb.x, cgb.y, cxb.z, cxb.w, cxc.x);
            apply(cgb.z, cgb.w, cxc.y, cxc.z, cxc.w);
        }
        if (rep == 0) {     // ragged tail (n % 4 samples)
            const int64_t i = n_full * 4 + threadIdx.x;
            if (i < n_live) { const float2 g = g_l[i]; apply(g.x, g.y, x01[3 * i], x01[3 * i + 1], x01[3 * i + 2]); }
        }
    } else {
        for (int64_t i = (int64_t)rep * kLnThreads + threadIdx.x; i < n_live; i += (int64_t)R * kLnThreads) {
            const float2 g = g_l[i];
            apply(g.x, g.y, x01[3 * i], x01[3 * i + 1], x01[3 * i + 2]);
        }
    }
    __syncthreads();
    // ---- LINE_OVERLAP: both copies of a shared vertex := the sum of their contributions (BEFORE the overflow test: folding can double
    //      a field).  The two entries lie in adjacent blocks of one super-block row, i.e. in this tile (2^(sb_shift[0] - 2) <= 512 blocks)
    if (gl.ovl) {
        const uint32_t runs_m = (1u << (gl.shx - 2)) - 1u;
        for (uint32_t j = threadIdx.x; j < kLnTileEntries; j += kLnThreads) {
            if ((j & 3u) != 3u || ((j >> 5) & runs_m) == runs_m) continue;
            const uint32_t j2 = j + 29u;
            if (FIXED) { const unsigned long long s = lds64[j] + lds64[j2]; lds64[j] = s; lds64[j2] = s; }
            else {
                const float s0 = lds[2 * j] + lds[2 * j2], s1 = lds[2 * j + 1] + lds[2 * j2 + 1];
                lds[2 * j] = s0; lds[2 * j + 1] = s1; lds[2 * j2] = s0; lds[2 * j2 + 1] = s1;
            }
        }
        __syncthreads();
    }
    // ---- write back (replicas: their integer / fp32 slabs)
    int32_t field_max = 0;
    const bool slab = R > 1;
    float2* out = slab ? ws + lp.ws_off[l] + (int64_t)rep * size : grad + gp.offset[l];
    const bool acc = !slab && lp.accumulate;
    const float2* src = reinterpret_cast<const float2*>(lds);
    for (uint32_t j = threadIdx.x; j < kLnTileEntries; j += kLnThreads) {
        const uint32_t e = (t << kLnTileShift) + j;
        if (e >= size) break;
        float2 v;
        if (FIXED) {
            const long long tot = (long long)lds64[j];
            const int32_t lo = (int32_t)(tot & 0xffffffffll);
            const int32_t hi = (int32_t)((tot - (long long)lo) >> 32);
            const int32_t alo = lo < 0 ? -(lo + 1) : lo, ahi = hi < 0 ? -(hi + 1) : hi;
            field_max = max(field_max, max(alo, ahi));
            if (slab) { reinterpret_cast<int2*>(out)[e] = make_int2(lo, hi); continue; }
            v = make_float2((float)lo * from_fixed, (float)hi * from_fixed);
        } else {
            v = src[j];
        }
        if (acc) { const float2 o = out[e]; v.x += o.x; v.y += o.y; }
        out[e] = v;
    }
#ifdef PERF_BWD_BLOCK_TIMES         // (two workgroups per level and replica report: a printf from every one stretches the launch)
    __syncthreads();
    if (FIXED && threadIdx.x == 0 && (t == 0u || t == (uint32_t)lp.tiles_of[l] / 2u))
        printf("BLOCKT_LINES level %d tile %u rep %d of %d ticks %lld\n", l, t, rep, R, wall_clock64() - block_t0);
#endif
    if (FIXED && overflow_flag && field_max >= (1 << 29)) atomicOr(overflow_flag, 1);
    if (FIXED && hr_state && !slab) {   // largest |field| of the level for the feedback: ONE atomic per workgroup
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) field_max = max(field_max, __shfl_xor(field_max, off));
        __shared__ int32_t wave_max[kLnThreads / 64];
        if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = field_max;
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t m = 0;
#pragma unroll
            for (int w = 0; w < kLnThreads / 64; ++w) m = max(m, wave_max[w]);
            if (m > 0) atomicMax(&hr_state[PERF_MAX_LEVELS + l], m);
        }
    }
}

// sum the replica slabs of the replicated line-local levels into the gradient table (fixed point: integer sums, any order)
__global__ __launch_bounds__(256) void hashgrid_bwd_lines_reduce_kernel(GridParams gp, LinesPlan lp, const float2* __restrict__ ws,
                                                                        float2* __restrict__ grad, const float* __restrict__ level_absmax,
                                                                        int32_t* __restrict__ hr_state, int32_t* __restrict__ overflow_flag,
                                                                        int fixed, int64_t n, const int64_t* __restrict__ n_dev) {
    const int l = blockIdx.y;
    const int R = lp.replicas_of[l];
    if (!((lp.owner_levels >> l) & 1u) || R <= 1) return;
    const uint32_t size = gp.size[l];
    const float from_fixed = fixed ? ldexpf(1.0f, -fixed_point_shift(level_absmax[l], live_count(n, n_dev), size, hr_state, l)) : 1.0f;
    int32_t field_max = 0;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < size; e += gridDim.x * 256) {
        float2* o = grad + gp.offset[l] + e;
        float fx, fy;
        if (fixed) {
            const int2* p = reinterpret_cast<const int2*>(ws + lp.ws_off[l]) + e;
            int32_t sx = 0, sy = 0;
            for (int r = 0; r < R; ++r) { const int2 v = p[(int64_t)r * size]; sx += v.x; sy += v.y; }
            const int32_t ax = sx < 0 ? -(sx + 1) : sx, ay = sy < 0 ? -(sy + 1) : sy;
            field_max = max(field_max, max(ax, ay));
            fx = (float)sx * from_fixed; fy = (float)sy * from_fixed;
        } else {
            const float2* p = ws + lp.ws_off[l] + e;
            fx = 0.f; fy = 0.f;
            for (int r = 0; r < R; ++r) { const float2 v = p[(int64_t)r * size]; fx += v.x; fy += v.y; }
        }
        if (lp.accumulate) { const float2 c = *o; fx += c.x; fy += c.y; }
        *o = make_float2(fx, fy);
    }
    if (fixed) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) field_max = max(field_max, __shfl_xor(field_max, off));
        if ((threadIdx.x & 63) == 0 && field_max > 0) {
            if (overflow_flag && field_max >= (1 << 29)) atomicOr(overflow_flag, 1);
            if (hr_state) atomicMax(&hr_state[PERF_MAX_LEVELS + l], field_max);
        }
    }
}

// Line-local levels beyond the owners: plain scatter with global atomics, the owners' weight association and units.  FIXED: the level's
// slice of the gradient table, zeroed by the caller, is an array of 64-bit words holding the packed fields (ONE atomic per corner and
// copy); hashgrid_bwd_lines_unfix_kernel turns them into float2 in place.  Otherwise two fp32 atomics per corner and copy (and
// hashgrid_bwd_lines_tie_kernel makes the copies bit-equal).
template <bool FIXED>
__global__ __launch_bounds__(256) void hashgrid_bwd_lines_scatter_kernel(GridParams gp, GridLocal gl, uint32_t levels, const float* __restrict__ x01,
                                                                        const float2* __restrict__ dfeat, float* __restrict__ grad,
                                                                        const float* __restrict__ level_absmax, const int32_t* __restrict__ hr_state,
                                                                        int64_t n, const int64_t* __restrict__ n_dev) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int l = blockIdx.y;
    const int64_t n_live = live_count(n, n_dev);
    if (i >= n_live || !((levels >> l) & 1u)) return;
    const float2 g = dfeat[(int64_t)l * n + i];
    if (g.x == 0.f && g.y == 0.f) return;
    const uint32_t size = gp.size[l];
    const float to_fixed = FIXED ? ldexpf(1.0f, fixed_point_shift(level_absmax[l], n_live, size, hr_state, l)) : 1.0f;
    const Corners c = corners_of_any(gp, gl, l, x01[3 * i], x01[3 * i + 1], x01[3 * i + 2]);
    float w[8];
    corner_weights(c.f, gp.interpolation == PERF_INTERP_SMOOTHSTEP, w);
    const float sx = g.x * to_fixed, sy = g.y * to_fixed;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t idx = c.idx[k];
        if (idx >= size) continue;          // (a dense level's cell far outside the unit cube)
        const uint32_t twin = gl.ovl ? overlap_twin(gl, idx) : 0xffffffffu;
        if (FIXED) {
            unsigned long long* t = reinterpret_cast<unsigned long long*>(grad) + gp.offset[l];
            const unsigned long long v = fixed_word(w[k], sx, sy);
            atomicAdd(t + idx, v);
            if (twin != 0xffffffffu) atomicAdd(t + twin, v);
        } else {
            float* t = grad + 2 * gp.offset[l];
            unsafeAtomicAdd(t + 2 * (uint64_t)idx, w[k] * g.x); unsafeAtomicAdd(t + 2 * (uint64_t)idx + 1, w[k] * g.y);
            if (twin != 0xffffffffu) { unsafeAtomicAdd(t + 2 * (uint64_t)twin, w[k] * g.x); unsafeAtomicAdd(t + 2 * (uint64_t)twin + 1, w[k] * g.y); }
        }
    }
}

__global__ __launch_bounds__(256) void hashgrid_bwd_lines_unfix_kernel(GridParams gp, uint32_t levels, float* __restrict__ grad,
                                                                       const float* __restrict__ level_absmax, int32_t* __restrict__ hr_state,
                                                                       int32_t* __restrict__ overflow_flag, int64_t n, const int64_t* __restrict__ n_dev) {
    const int l = blockIdx.y;
    if (!((levels >> l) & 1u)) return;
    const uint32_t size = gp.size[l];
    const float from_fixed = ldexpf(1.0f, -fixed_point_shift(level_absmax[l], live_count(n, n_dev), size, hr_state, l));
    unsigned long long* t = reinterpret_cast<unsigned long long*>(grad) + gp.offset[l];
    int32_t field_max = 0;
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < size; e += gridDim.x * 256) {
        const long long tot = (long long)t[e];
        if (tot == 0) continue;
        const int32_t lo = (int32_t)(tot & 0xffffffffll);
        const int32_t hi = (int32_t)((tot - (long long)lo) >> 32);
        reinterpret_cast<float2*>(t)[e] = make_float2((float)lo * from_fixed, (float)hi * from_fixed);
        const int32_t alo = lo < 0 ? -(lo + 1) : lo, ahi = hi < 0 ? -(hi + 1) : hi;
        field_max = max(field_max, max(alo, ahi));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) field_max = max(field_max, __shfl_xor(field_max, off));
    if ((threadIdx.x & 63) == 0 && field_max > 0) {
        if (overflow_flag && field_max >= (1 << 29)) atomicOr(overflow_flag, 1);
        if (hr_state) atomicMax(&hr_state[PERF_MAX_LEVELS + l], field_max);
    }
}

// fp32 scatter of a LINE_OVERLAP level: both copies of a shared vertex received the same updates, summed in another order -- the
// second copy takes the first one's value, so that the copies are bit-equal as the owners leave them
__global__ __launch_bounds__(256) void hashgrid_bwd_lines_tie_kernel(GridParams gp, GridLocal gl, uint32_t levels, float2* __restrict__ grad) {
    const int l = blockIdx.y;
    if (!((levels >> l) & 1u)) return;
    float2* t = grad + gp.offset[l];
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < gp.size[l]; e += gridDim.x * 256)
        if ((e & 3u) == 3u && overlap_twin(gl, e) != 0xffffffffu) t[e + 29u] = t[e];
}

// headroom feedback of the line-local levels (the tcnn-rule prefix got its own from perf_internal_hashgrid_bwd): a launch of its own,
// behind every launch that raised the levels' maxima
__global__ __launch_bounds__(64) void hashgrid_bwd_lines_feedback_kernel(uint32_t levels, int32_t* __restrict__ hr_state) {
    const int l = threadIdx.x;
    if (l >= PERF_MAX_LEVELS || !((levels >> l) & 1u)) return;
    hr_state[l] = headroom_feedback(hr_state[l], hr_state[PERF_MAX_LEVELS + l]);
    hr_state[PERF_MAX_LEVELS + l] = 0;
}

__global__ void step_book_keep_flag_lines_kernel(perf_step_book b) { step_bookkeeping_thread(b, false); }

}  // namespace perf

using namespace perf;

static void step_book_keep_flag_lines_launch(const perf_step_book& b, void* stream) {
    hipLaunchKernelGGL(perf::step_book_keep_flag_lines_kernel, dim3(1), dim3(1), 0, as_stream(stream), b);
}

// the prefix descriptor (tcnn-rule levels 0..P-1) and the line-local suffix check; returns P or -1
static int split_lines(const perf_grid_desc* grid, GridParams* gp, GridLocal* gl, perf_grid_desc* prefix) {
    PERF_REQUIRE(grid != nullptr, "grid desc is NULL");
    if (grid->layout == PERF_LAYOUT_TCNN) {
        set_error("perf_hashgrid_bwd_lines takes PERF_LAYOUT_LINE_LOCAL / _OVERLAP grids; a tcnn-layout grid goes through perf_hashgrid_bwd");
        return -1;
    }
    if (fill_params(grid, gp, gl)) return -1;
    int P = 0;
    while (P < gp->n_levels && !gl->local[P]) ++P;
    for (int l = P; l < gp->n_levels; ++l)
        if (!gl->local[l]) { set_error("perf_hashgrid_bwd_lines: level %d is not line-local but level %d is (line-local levels must be a suffix)", l, P); return -1; }
    if (gl->ovl && (1u << (gl->shx - 2)) > 512u) {
        set_error("perf_hashgrid_bwd_lines: line_overlap needs 2^(sb_shift[0] - 2) <= 512 blocks per super-block row (both copies of a shared vertex in one tile)");
        return -1;
    }
    *prefix = *grid;
    prefix->n_levels = P;
    prefix->layout = PERF_LAYOUT_TCNN;
    return P;
}

// the ONE layout of what the line-local owners take at the END of the workspace: [16][replica slabs][tile codes of n samples]
struct LinesTail { int64_t owners, coded; };       // bytes without / with the tile codes (which start `owners` bytes into the tail)
static LinesTail lines_tail(const GridParams& gp, const GridLocal& gl, int64_t n) {
    LinesPlan lp; int64_t slab = 0;
    plan_lines(gp, gl, true, true, &lp, &slab);
    int levels = 0;
    for (int l = 0; l < gp.n_levels; ++l) levels += (lp.owner_levels >> l) & 1u;
    const int64_t owners = 16 + ((slab * (int64_t)sizeof(float2) + 15) & ~(int64_t)15);
    return {owners, owners + (int64_t)levels * ((n + 1) & ~(int64_t)1) * 8};
}

// the padding in front of a line-local level (it starts on a super-block boundary) is part of the table: an overwriting call writes 0
static int zero_padding(const GridParams& gp, const GridLocal& gl, float* grad, void* stream) {
    for (int l = 1; l < gp.n_levels; ++l) {
        const uint64_t end = gp.offset[l - 1] + gp.size[l - 1];
        if (gl.local[l] && gp.offset[l] > end)
            PERF_REQUIRE(hipMemsetAsync(grad + 2 * end, 0, (size_t)(gp.offset[l] - end) * 2 * sizeof(float), as_stream(stream)) == hipSuccess,
                         "perf_hashgrid_bwd_lines: memset failed");
    }
    return PERF_OK;
}

extern "C" int64_t perf_hashgrid_bwd_lines_workspace_bytes(const perf_grid_desc* grid, int64_t n) {
    GridParams gp; GridLocal gl; perf_grid_desc pre;
    const int P = split_lines(grid, &gp, &gl, &pre);
    if (P < 0 || n < 0) return -1;
    int64_t a = 0;
    if (P > 0) { a = perf_hashgrid_bwd_workspace_bytes(&pre, n); if (a < 0) return -1; }
    return ((a + 15) & ~(int64_t)15) + lines_tail(gp, gl, n).coded;
}

extern "C" int perf_hashgrid_bwd_lines(const perf_grid_desc* grid, const float* x01, const float* dfeat, float* grad_table, int64_t n,
                                       const int64_t* n_dev, int accumulate, const float* level_absmax, int32_t* overflow_flag,
                                       int32_t* headroom_state, const int32_t* shifts_dev, int raw_fields, const int32_t* redo_flag,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    return perf_internal_hashgrid_bwd_lines(grid, x01, dfeat, grad_table, n, n_dev, accumulate, level_absmax, overflow_flag, headroom_state,
                                            shifts_dev, raw_fields, redo_flag, workspace, workspace_bytes, stream, nullptr, nullptr);
}

int perf_internal_hashgrid_bwd_lines(const perf_grid_desc* grid, const float* x01, const float* dfeat, float* grad_table, int64_t n,
                                     const int64_t* n_dev, int accumulate, const float* level_absmax, int32_t* overflow_flag,
                                     int32_t* headroom_state, const int32_t* shifts_dev, int raw_fields, const int32_t* redo_flag,
                                     void* workspace, int64_t workspace_bytes, void* stream, const MlpReduceJob* job_in,
                                     const perf_step_book* book) {
    GridParams gp; GridLocal gl; perf_grid_desc pre;
    const int P = split_lines(grid, &gp, &gl, &pre);
    if (P < 0) return PERF_E_INVALID;
    PERF_REQUIRE(!shifts_dev && !raw_fields,
                 "perf_hashgrid_bwd_lines: given units (shifts_dev) / raw fields (the data-parallel integer exchange) are not available for line-local layouts");
    PERF_REQUIRE(!book || redo_flag, "perf_hashgrid_bwd_lines: the bookkeeping rides in a repair launch only");
    PERF_REQUIRE(grad_table, "NULL pointer");
    PERF_REQUIRE(n >= 0 && (n == 0 || (x01 && dfeat)), "NULL pointer");
    const bool fixed = level_absmax != nullptr;
    const uint32_t local_levels = (gp.n_levels >= 32 ? 0xffffffffu : ((1u << gp.n_levels) - 1u)) & ~((1u << P) - 1u);
    const int lds_bytes = 2 * (int)kLnTileEntries * (int)sizeof(float) + (kLnThreads / 64) * kLnQueueCap * (int)sizeof(uint32_t);
    static std::once_flag attr_once;
    std::call_once(attr_once, [&]() {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&hashgrid_bwd_lines_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&hashgrid_bwd_lines_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    });
    if (redo_flag) {
        // the repair of a fixed-point call whose fields overflowed: the prefix's own repair launch, then fp32 owners without replicas for
        // the line-local levels, both predicated on the flag
        PERF_REQUIRE(!fixed && !accumulate, "perf_hashgrid_bwd_lines: a redo call is an fp32, overwriting call");
        LinesPlan rp; int64_t slab = 0;
        plan_lines(gp, gl, true, false, &rp, &slab);
        if (rp.atomic_levels != 0u) { set_error("perf_hashgrid_bwd_lines: the redo launch serves grids whose line-local levels all fit LDS owners (<= 255 tiles)"); return PERF_E_UNSUPPORTED; }
        if (zero_padding(gp, gl, grad_table, stream)) return PERF_E_LAUNCH;
        if (P > 0) {
            const int rc = perf_internal_hashgrid_bwd(&pre, x01, dfeat, grad_table, n, n_dev, 0, nullptr, nullptr, headroom_state, nullptr, 0, redo_flag,
                                                      nullptr, 0, stream, nullptr, book);
            if (rc) return rc;
        }
        if (n > 0 && rp.n_blocks > 0)
            hashgrid_bwd_lines_kernel<false><<<dim3(rp.n_blocks), dim3(kLnThreads), lds_bytes, as_stream(stream)>>>(
                gp, gl, rp, x01, (const float2*)dfeat, (float2*)grad_table, nullptr, nullptr, nullptr, P == 0 ? headroom_state : nullptr, n, n_dev,
                redo_flag, (P == 0 && book) ? *book : perf_step_book{}, (P == 0 && book) ? 1 : 0, nullptr);
        else if (P == 0 && book)
            step_book_keep_flag_lines_launch(*book, stream);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(redo)");
        return PERF_OK;
    }
    // workspace: [the prefix's (perf_hashgrid_bwd_workspace_bytes)][16][line-local replica slabs]; without room for the tail every
    // line-local level takes the global-atomics scatter (and the prefix gets the whole workspace)
    // (a workspace with room for the slabs but not for the tile codes selects the position-streaming owners)
    const LinesTail lt = lines_tail(gp, gl, n);
    int64_t pre_min = 0;
    if (P > 0) { pre_min = perf_hashgrid_bwd_workspace_bytes(&pre, 0); if (pre_min < 0) return PERF_E_INVALID; }
    pre_min = (pre_min + 15) & ~(int64_t)15;
    const bool aligned_ws = workspace && ((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
    const bool coded = aligned_ws && n > 0 && workspace_bytes >= pre_min + lt.coded;
    const bool owners = aligned_ws && workspace_bytes >= pre_min + lt.owners;
    const int64_t slab_at = owners ? ((workspace_bytes - (coded ? lt.coded : lt.owners)) & ~(int64_t)15) : workspace_bytes;
    float2* slabs = owners ? reinterpret_cast<float2*>(reinterpret_cast<char*>(workspace) + slab_at + 16) : nullptr;
    LinesPlan lp; int64_t slab_entries = 0;
    plan_lines(gp, gl, owners, true, &lp, &slab_entries);
    unsigned long long* codes = nullptr;
    if (coded) {
        codes = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + slab_at + lt.owners);
        lp.n_pad = (n + 1) & ~(int64_t)1;
        int slot = 0;
        for (int l = 0; l < gp.n_levels; ++l) if ((lp.owner_levels >> l) & 1u) lp.code_slot[l] = slot++;
    }
    lp.accumulate = accumulate ? 1 : 0;
    if (!accumulate && zero_padding(gp, gl, grad_table, stream)) return PERF_E_LAUNCH;
    if (P > 0) {
        const int rc = perf_internal_hashgrid_bwd(&pre, x01, dfeat, grad_table, n, n_dev, accumulate, level_absmax, overflow_flag, headroom_state,
                                                  nullptr, 0, nullptr, workspace, slab_at, stream, job_in, nullptr);
        if (rc) return rc;
    } else if (job_in && job_in->n_blocks) {        // (the MLP backward's deferred second stage: before the owners, which read level_absmax)
        perf_internal_launch_mlp_reduce(*job_in, stream);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(deferred MLP reduce)");
    }
    if (lp.n_blocks > 0) {
        if (codes) {
            hashgrid_bwd_lines_codes_kernel<<<dim3((unsigned)div_up(n, 256), gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                gp, gl, lp, x01, (const float2*)dfeat, codes, n, n_dev);
            PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(codes)");
        }
        if (fixed)
            hashgrid_bwd_lines_kernel<true><<<dim3(lp.n_blocks), dim3(kLnThreads), lds_bytes, as_stream(stream)>>>(
                gp, gl, lp, x01, (const float2*)dfeat, (float2*)grad_table, slabs, level_absmax, overflow_flag, headroom_state, n, n_dev,
                nullptr, perf_step_book{}, 0, codes);
        else
            hashgrid_bwd_lines_kernel<false><<<dim3(lp.n_blocks), dim3(kLnThreads), lds_bytes, as_stream(stream)>>>(
                gp, gl, lp, x01, (const float2*)dfeat, (float2*)grad_table, slabs, nullptr, nullptr, nullptr, n, n_dev, nullptr, perf_step_book{}, 0,
                codes);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines");
        bool any_rep = false;
        for (int l = 0; l < gp.n_levels; ++l) any_rep = any_rep || lp.replicas_of[l] > 1;
        if (any_rep) {
            hashgrid_bwd_lines_reduce_kernel<<<dim3(64, gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                gp, lp, slabs, (float2*)grad_table, level_absmax, fixed ? headroom_state : nullptr, fixed ? overflow_flag : nullptr, fixed ? 1 : 0, n, n_dev);
            PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(reduce)");
        }
    }
    const bool fixed_atomics = fixed && !accumulate && (reinterpret_cast<uintptr_t>(grad_table) & 7) == 0;
    if (lp.atomic_levels) {
        if (!accumulate)
            for (int l = 0; l < gp.n_levels; ++l)
                if ((lp.atomic_levels >> l) & 1u)
                    PERF_REQUIRE(hipMemsetAsync(grad_table + 2 * gp.offset[l], 0, (size_t)gp.size[l] * 2 * sizeof(float), as_stream(stream)) == hipSuccess,
                                 "perf_hashgrid_bwd_lines: memset failed");
        if (n > 0) {
            if (fixed_atomics) {
                hashgrid_bwd_lines_scatter_kernel<true><<<dim3((unsigned)div_up(n, 256), gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                    gp, gl, lp.atomic_levels, x01, (const float2*)dfeat, grad_table, level_absmax, headroom_state, n, n_dev);
                PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(atomics, fixed point)");
                hashgrid_bwd_lines_unfix_kernel<<<dim3(1024, gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                    gp, lp.atomic_levels, grad_table, level_absmax, headroom_state, overflow_flag, n, n_dev);
                PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(unfix)");
            } else {
                hashgrid_bwd_lines_scatter_kernel<false><<<dim3((unsigned)div_up(n, 256), gp.n_levels), dim3(256), 0, as_stream(stream)>>>(
                    gp, gl, lp.atomic_levels, x01, (const float2*)dfeat, grad_table, nullptr, nullptr, n, n_dev);
                PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(atomics)");
                if (gl.ovl) {
                    hashgrid_bwd_lines_tie_kernel<<<dim3(1024, gp.n_levels), dim3(256), 0, as_stream(stream)>>>(gp, gl, lp.atomic_levels, (float2*)grad_table);
                    PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(copies)");
                }
            }
        }
    }
    if (fixed && headroom_state) {
        // (levels that took the fp32 scatter -- accumulate, or an unaligned table -- recorded no field maxima: no feedback for them)
        const uint32_t fed = lp.owner_levels | (fixed_atomics ? lp.atomic_levels : 0u);
        hashgrid_bwd_lines_feedback_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(fed & local_levels, headroom_state);
        PERF_LAUNCH_CHECK("perf_hashgrid_bwd_lines(feedback)");
    }
    return PERF_OK;
}
