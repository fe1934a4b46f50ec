// Occupancy-grid ray marching (nerfacc traverse_grids semantics as restated in SURVEY.md A.3 and
// oracle/perf_oracle.py:occ_march) for gfx950.
//
// One 64-lane wavefront owns one ray.  Lane k of chunk q tests lattice interval 64*q+k: the 64
// midpoints of a chunk are consecutive points on the ray, so their occupancy words are neighbours
// in the bit field (256^3 bits = 2 MiB: L2 resident).  A wave ballot turns the 64 tests into one
// uint64 keep-mask; pass 1 stores the masks and the per-ray popcount, an exclusive scan over rays
// gives the packed offsets, pass 2 expands the masks with a per-lane prefix popcount -- the
// "count -> scan -> write" protocol with bit-exact, t-sorted output and no atomics.
// All lattice/cell arithmetic is unfused fp32 (mul_rn/add_rn) so it matches numpy bit for bit.
#include <cstring>

#include "common.hpp"
#include "step_riders_device.hpp"

namespace perf {

__global__ __launch_bounds__(256) void coarse_build_kernel(const uint32_t* __restrict__ bits, int res,
                                                           uint32_t* __restrict__ coarse) {
    constexpr int B = kCoarseBlock;
    const int cr = res / B;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= cr * cr * cr) return;
    const int bx = b / (cr * cr), by = (b / cr) % cr, bz = b % cr;
    bool any = false;
    for (int x = max(bx - 1, 0) * B; x < min(bx + 2, cr) * B && !any; ++x)
        for (int y = max(by - 1, 0) * B; y < min(by + 2, cr) * B && !any; ++y) {
            // the z run [z0, z1) of a row is contiguous in the bit field (B divides 32: a block's run never straddles a word)
            const int z0 = max(bz - 1, 0) * B, z1 = min(bz + 2, cr) * B;
            for (int z = z0; z < z1; z += B) {
                const uint32_t ci = (uint32_t)((x * res + y) * res + z);
                if ((bits[ci >> 5] >> (ci & 31)) & ((1u << B) - 1u)) { any = true; break; }
            }
        }
    if (any) atomicOr(&coarse[b >> 5], 1u << (b & 31));
}

__global__ __launch_bounds__(256) void fine_build_kernel(const uint32_t* __restrict__ bits, int res, uint32_t* __restrict__ fine) {
    constexpr int B = kFineBlock;
    const int fr = res / B;
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= (int64_t)fr * fr * fr) return;
    const int bx = (int)(b / ((int64_t)fr * fr)), by = (int)((b / fr) % fr), bz = (int)(b % fr);
    bool any = false;
    const int z0 = max(bz - 1, 0) * B, z1 = min(bz + 2, fr) * B;
    for (int x = max(bx - 1, 0) * B; x < min(bx + 2, fr) * B && !any; ++x)
        for (int y = max(by - 1, 0) * B; y < min(by + 2, fr) * B && !any; ++y)
            for (int z = z0; z < z1; z += B) {                       // (B divides 32: a block's z run never straddles a word)
                const uint32_t ci = (uint32_t)((x * res + y) * res + z);
                if ((bits[ci >> 5] >> (ci & 31)) & ((1u << B) - 1u)) { any = true; break; }
            }
    if (any) atomicOr(&fine[b >> 5], 1u << (b & 31));
}

static inline uint32_t host_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float host_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static void shared_runs_build(float t0, float step, int k_need, SharedRuns* sr) {
    sr->n = 0;
    int n = 0;
    auto emit = [&](int k, uint32_t b, uint32_t d) { sr->ks[n] = k; sr->bs[n] = b; sr->dd[n] = d; ++n; };
    uint32_t tb = host_bits(t0);
    emit(0, tb, 0u);
    int K = 0;
    while (K < k_need) {
        if (n + 2 > kMaxRuns) return;                            // (too many binades for the table: the kernels walk per lane)
        volatile float s1 = host_float(tb) + step;               // (volatile: one rounding to fp32 per addition, whatever the host compiler does)
        const uint32_t b1 = host_bits(s1);
        if ((b1 >> 23) != (tb >> 23)) { emit(K + 1, b1, 0u); tb = b1; K += 1; continue; }
        volatile float s2 = host_float(b1) + step;
        const uint32_t b2 = host_bits(s2);
        if ((b2 >> 23) != (b1 >> 23)) { emit(K + 1, b1, 0u); emit(K + 2, b2, 0u); tb = b2; K += 2; continue; }
        const uint32_t d = b2 - b1;
        emit(K + 1, b1, d);
        if (d == 0u) break;
        const uint32_t top = (b2 & 0xff800000u) + 0x00800000u;
        const uint32_t j = (top - 1u - b2) / d;
        tb = b2 + j * d;
        K += 2 + (int)j;
    }
    sr->n = n;
}

template <bool HEAD>
__global__ __launch_bounds__(256) void march_count_kernel(MarchParams mp, const float* __restrict__ ro,
                                                          const float* __restrict__ rd, const float* __restrict__ t0s,
                                                          int64_t n_rays, const uint32_t* __restrict__ bits,
                                                          const uint32_t* __restrict__ coarse,
                                                          uint64_t* __restrict__ masks, int32_t* __restrict__ counts, HeadOut ho,
                                                          float t0_scale, float t0_base, SharedRuns sr, const float* __restrict__ lat_full) {
    march_count_body<HEAD>((int)blockIdx.x, mp, ro, rd, t0s, n_rays, bits, coarse, masks, counts, ho, t0_scale, t0_base, sr, lat_full);
}

// ---- large launches on ONE lattice (eval frames: no jitter, t_k precomputed): a ray per LANE for everything that is uniform
// per ray.  The wave-per-ray kernel above is VALU bound on such launches -- 488 vector instructions per ray on a 524,288-ray
// frame (SQ_ACTIVE_INST_VALU 95 %), of which ~140 are the ray's set-up (slab test with three IEEE divisions, skip-grid validity)
// executed by 64 lanes on uniform values and ~100 the chunk ballot that uses 47 of 64 lanes.  Here a wave takes 64 rays: set-up
// and the chunk decisions (range + dilated coarse grid; the chunk's lattice points are the same for every ray: scalar loads)
// run lane-parallel -- the coarse-grid words of eight chunks in flight per round --, then the wave walks its rays' surviving
// chunks exactly as above (64 intervals of a chunk, one per lane).  Same arithmetic per ray, same masks, counts and head rows.
// Needs enough rays to fill the chip with 64-ray waves (the host picks it from kSharedMinRays rays on) and one live word per
// ray (max_steps <= 4096).
constexpr int64_t kSharedMinRays = 262144;
constexpr int kSharedHeadMax = 16;                 // head rows per ray this kernel can hold (the host's STRIDED_HEAD_MAX)
template <bool HEAD>
__global__ __launch_bounds__(64) void march_count_shared_kernel(MarchParams mp, const float* __restrict__ ro, const float* __restrict__ rd,
                                                                int64_t n_rays, const uint32_t* __restrict__ bits,
                                                                const uint32_t* __restrict__ coarse, uint64_t* __restrict__ masks,
                                                                int32_t* __restrict__ counts, HeadOut ho, float t0_base,
                                                                const float* __restrict__ lat_full) {
    __shared__ int32_t s_head[HEAD ? 64 * kSharedHeadMax : 1];                // [ray of the wave][rank]: lattice index of the ray's first K samples
    const int lane = threadIdx.x;
    const int64_t r_base = (int64_t)blockIdx.x * 64;
    const int res = mp.res;
    const float rf = (float)res;
    // ---- per lane: the ray's range and its chunk decisions
    uint64_t live_mine = 0;
    float lo_mine = 0.f, hi_mine = 0.f;
    {
        const int64_t r = r_base + lane;
        if (r < n_rays) {
            const float o[3] = {ro[3 * r], ro[3 * r + 1], ro[3 * r + 2]};
            const float d[3] = {rd[3 * r], rd[3 * r + 1], rd[3 * r + 2]};
            float tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float inv = __fdiv_rn(1.0f, d[a]);
                const float t1 = mul_rn(sub_rn(mp.lo[a], o[a]), inv), t2 = mul_rn(sub_rn(mp.hi[a], o[a]), inv);
                const float l = fminf(t1, t2), h = fmaxf(t1, t2);
                tmin = (a == 0) ? l : fmaxf(tmin, l);
                tmax = (a == 0) ? h : fminf(tmax, h);
            }
            lo_mine = fmaxf(tmin, t0_base); hi_mine = fminf(tmax, mp.far_plane);
            float span_cells = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) span_cells = fmaxf(span_cells, fabsf(d[a]) * mp.chunk_cells[a]);
            const bool use_coarse = mp.use_coarse && (span_cells * 0.5f + 1.5f <= (float)kCoarseBlock);
            const bool use_fine = use_coarse && (span_cells * (16.5f / 64.0f) + 0.5f <= (float)kFineBlock);
            const uint32_t* fine = coarse ? coarse + coarse_words_of(res) : nullptr;
            const int fr = res >> kFineShift;
            const int cr = res >> kCoarseShift;
            for (int q0 = 0; q0 < mp.mask_words; q0 += 8) {
                uint32_t bi[8]; bool in[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u;
                    bi[u] = 0u; in[u] = false;
                    if (q < mp.mask_words) {                                 // (uniform)
                        const int k0 = q * 64;
                        const float t_first = lat_full[k0], t_mid = lat_full[k0 + 32], t_last = lat_full[k0 + 64];     // (uniform addresses)
                        in[u] = !(t_first > hi_mine) && !(t_last < lo_mine);
                        if (in[u] && use_coarse) {
                            int cb[3];
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                const float p = add_rn(o[a], mul_rn(d[a], t_mid));
                                const float uu = mul_rn(mul_rn(sub_rn(p, mp.lo[a]), mp.inv_ext[a]), rf);
                                cb[a] = ((int)fminf(fmaxf(floorf(uu), 0.0f), rf - 1.0f)) >> kCoarseShift;
                            }
                            bi[u] = (uint32_t)((cb[0] * cr + cb[1]) * cr + cb[2]);
                        }
                    }
                }
                uint32_t w[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) w[u] = (in[u] && use_coarse) ? coarse[bi[u] >> 5] : 0u;
                // survivors of the coarse test: the fine grid at two lattice points of the chunk (few per ray: a divergent tail)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    bool alive = in[u] && (!use_coarse || ((w[u] >> (bi[u] & 31u)) & 1u));
                    if (alive && use_fine) {
                        const int k0 = (q0 + u) * 64;
                        const uint32_t f1 = fine_block_at(mp, o, d, lat_full[k0 + 16], rf, fr);
                        const uint32_t f3 = fine_block_at(mp, o, d, lat_full[k0 + 48], rf, fr);
                        alive = (((fine[f1 >> 5] >> (f1 & 31)) | (fine[f3 >> 5] >> (f3 & 31))) & 1u) != 0u;
                    }
                    if (alive) live_mine |= 1ull << (q0 + u);
                }
            }
        }
    }
    // ---- the wave walks its rays.  What a ray leaves behind besides its chunk masks -- the record's first word, its count, its head rows
    //      -- is kept by the ray's LANE and written after the walk by all lanes at once: one pass of coalesced stores and lane-parallel
    //      sample_point_store instead of 64 single-lane tails (~55 of the ~310 vector instructions per ray were that tail)
    const uint32_t live_lo32 = (uint32_t)live_mine, live_hi32 = (uint32_t)(live_mine >> 32);
    char* rec_wave = reinterpret_cast<char*>(masks + r_base * (int64_t)(mp.mask_words + 1));
    const uint32_t rec_stride = (uint32_t)__builtin_amdgcn_readfirstlane((mp.mask_words + 1) * 8);       // (a scalar: s * rec_stride stays on the scalar unit)
    int32_t count_mine = 0;
    uint32_t kept_lo = 0u, kept_hi = 0u;
    for (int s = 0; s < 64; ++s) {
        const int64_t r = r_base + s;
        if (r >= n_rays) break;
        const uint64_t live = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)live_lo32, s) |
                              ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)live_hi32, s) << 32);
        if (!live) continue;                                         // (count_mine / kept of that lane stay 0)
        const float lo = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(lo_mine), s));
        const float hi = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(hi_mine), s));
        // (the record of ray s from the wave's base + a 32-bit offset: formed as r * (mask_words + 1) the compiler multiplied 64-bit
        //  integers on the vector unit for every ray)
        char* rec = rec_wave + (uint32_t)s * rec_stride;
        int32_t count = 0;
        uint64_t kept = 0;
        const float o[3] = {ro[3 * r], ro[3 * r + 1], ro[3 * r + 2]};
        const float d[3] = {rd[3 * r], rd[3 * r + 1], rd[3 * r + 2]};
        for (uint64_t todo = live; todo;) {
            int qs[4]; uint32_t cis[4]; bool in_range[4]; float ta[4];
            // the lattice points of up to four surviving chunks are requested TOGETHER (as written before -- one load inside each chunk's
            // branch -- every chunk waited for its own round trip); the table holds 64 points beyond the last chunk: no bound test here
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                qs[u] = -1; ta[u] = 0.f;
                if (todo) {
                    qs[u] = __ffsll((unsigned long long)todo) - 1;
                    todo &= todo - 1;
                    ta[u] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(lat_full) + (((uint32_t)qs[u] * 64u + (uint32_t)lane) << 2));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                cis[u] = 0u; in_range[u] = false;
                if (qs[u] < 0) continue;                 // (wave uniform)
                const int k = qs[u] * 64 + lane;
                if (k < mp.max_steps) {
                    const float tb = mp.lattice_mode == PERF_LATTICE_REPEATED ? add_rn(ta[u], mp.step) : lattice_single(t0_base, k + 1, mp.step);
                    const float mid = mul_rn(add_rn(ta[u], tb), 0.5f);
                    if (mid >= lo && mid <= hi) {
                        uint32_t cell[3];
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const float p = add_rn(o[a], mul_rn(d[a], mid));
                            const float uu = mul_rn(mul_rn(sub_rn(p, mp.lo[a]), mp.inv_ext[a]), rf);
                            cell[a] = (uint32_t)(int)fminf(fmaxf(floorf(uu), 0.0f), rf - 1.0f);
                        }
                        // (res <= 1024: both products fit 24-bit operands -- two full-rate multiply-adds instead of two 64-bit ones)
                        cis[u] = (uint32_t)__umul24((uint32_t)__umul24(cell[0], (uint32_t)res) + cell[1], (uint32_t)res) + cell[2];
                        in_range[u] = true;
                    }
                }
            }
            uint32_t words[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                words[u] = in_range[u] ? *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(bits) + ((cis[u] >> 5) << 2)) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (qs[u] < 0) continue;                 // (wave uniform)
                const bool mine = in_range[u] && ((words[u] >> (cis[u] & 31)) & 1u);
                const uint64_t m = __ballot(mine);
                if (m) {
                    kept |= 1ull << qs[u];
                    if (lane == 0) *reinterpret_cast<uint64_t*>(rec + ((uint32_t)(1 + qs[u]) << 3)) = m;
                    if (HEAD && count < ho.K && mine) {
                        const int rank = count + __popcll(m & ((1ull << lane) - 1ull));
                        if (rank < ho.K) s_head[s * kSharedHeadMax + rank] = qs[u] * 64 + lane;
                    }
                    count += __popcll(m);
                }
            }
        }
        if (lane == s) { count_mine = count; kept_lo = (uint32_t)kept; kept_hi = (uint32_t)(kept >> 32); }
    }
    // ---- per lane again: record heads, counts, head rows
    const int64_t r = r_base + lane;
    if (r >= n_rays) return;
    masks[r * (int64_t)(mp.mask_words + 1)] = (uint64_t)kept_lo | ((uint64_t)kept_hi << 32);
    counts[r] = count_mine;
    if (HEAD) {
        const int have = count_mine < ho.K ? count_mine : ho.K;
        ho.packed[2 * r] = (int32_t)(r * ho.K); ho.packed[2 * r + 1] = have;
        for (int j = 0; j < ho.K; ++j) {                             // (row j of 64 rays at a time)
            const int64_t pos = r * ho.K + j;
            if (j < have) {
                const int k = s_head[lane * kSharedHeadMax + j];
                const float a = lat_full[k], b = mp.lattice_mode == PERF_LATTICE_REPEATED ? add_rn(a, mp.step) : lattice_single(t0_base, k + 1, mp.step);
                ho.ts[pos] = a; ho.te[pos] = b; ho.ri[pos] = r;
                sample_point_store(ro + 3 * r, rd + 3 * r, a, b, ho.bb, ho.x01, ho.sel, pos);
            } else {                                                 // padding rows: harmless inputs, selector 0
                ho.ts[pos] = 0.f; ho.te[pos] = 0.f; ho.ri[pos] = r;
                ho.x01[3 * pos] = 0.5f; ho.x01[3 * pos + 1] = 0.5f; ho.x01[3 * pos + 2] = 0.5f; ho.sel[pos] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void march_write_kernel(const float* __restrict__ t0s, int64_t n_rays, float step,
                                                          int32_t mask_words, const uint64_t* __restrict__ masks,
                                                          const int32_t* __restrict__ counts,
                                                          const int32_t* __restrict__ offsets, int64_t capacity,
                                                          int64_t* __restrict__ ray_indices, float* __restrict__ ts,
                                                          float* __restrict__ te, int32_t* __restrict__ packed,
                                                          const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                          Aabb bb, float* __restrict__ x01, uint8_t* __restrict__ sel,
                                                          int32_t rank_lo, float t0_scale, float t0_base, int lattice_mode, SharedRuns sr,
                                                          const float* __restrict__ lat_full) {
    march_write_body((int)blockIdx.x, (int)gridDim.x, t0s, n_rays, step, mask_words, masks, counts, offsets, capacity, ray_indices, ts, te, packed, rays_o, rays_d,
                     bb, x01, sel, rank_lo, t0_scale, t0_base, lattice_mode, sr, lat_full);
}

// Large launches on ONE lattice (eval frames, as march_count_shared_kernel): a wave takes 64 rays.  Every ray's LANE reads its count and
// offset and stores its packed_info pair -- coalesced -- and the wave then walks only the rays that HAVE samples to write, four at a
// time on quarter waves (or one after the other with all 64 lanes when one of the four writes more than 16 samples).  On an eval frame of a trained scene most rays end inside their head (the two-phase sampler's tail
// counts are zero): march_write_kernel gave each of them a quarter wave that loaded two words, stored two and retired.  Same rows,
// same values.
__global__ __launch_bounds__(256) void march_write_shared_kernel(int64_t n_rays, float step, int32_t mask_words, const uint64_t* __restrict__ masks,
                                                                 const int32_t* __restrict__ counts, const int32_t* __restrict__ offsets,
                                                                 int64_t capacity, int64_t* __restrict__ ray_indices, float* __restrict__ ts,
                                                                 float* __restrict__ te, int32_t* __restrict__ packed,
                                                                 const float* __restrict__ rays_o, const float* __restrict__ rays_d, Aabb bb,
                                                                 float* __restrict__ x01, uint8_t* __restrict__ sel, int32_t rank_lo,
                                                                 float t0_base, int lattice_mode, const float* __restrict__ lat_full) {
    const int lane = threadIdx.x & 63;
    const int64_t r_base = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * 64;
    if (r_base >= n_rays) return;
    const int64_t rl = r_base + lane;
    int32_t cnt_mine = 0, off_mine = 0;
    if (rl < n_rays) {
        cnt_mine = counts[rl]; off_mine = offsets[rl];
        if ((int64_t)off_mine + cnt_mine > capacity) cnt_mine = (int32_t)(capacity > off_mine ? capacity - off_mine : 0);   // truncated batch
        packed[2 * rl] = off_mine; packed[2 * rl + 1] = cnt_mine;
    }
    const int nlw = n_live_words(mask_words);
    // one ray's samples, by a team of W lanes that walks the 64 bits of a mask word in 64 / W steps (march_write_kernel's loop)
    auto walk = [&](auto wc, int64_t r, int32_t cnt, int32_t off, int l) {
        constexpr int W = decltype(wc)::value;
        int64_t run = (int64_t)off - rank_lo;            // output position of rank 0 (may lie before `off`)
        const int64_t end = (int64_t)off + cnt;
        const uint64_t* rec = masks + r * (int64_t)(mask_words + nlw);
        for (int g = 0; g < nlw && run < end; ++g) {
            for (uint64_t todo = rec[g]; todo && run < end; todo &= todo - 1) {
                const int qq = g * 64 + (__ffsll((unsigned long long)todo) - 1);
                const uint64_t m = rec[nlw + qq];
                for (int bit = l; bit < 64; bit += W) {
                    if (!((m >> bit) & 1ull)) continue;
                    const uint64_t below = (bit == 0) ? 0ull : (~0ull >> (64 - bit));
                    const int64_t pos = run + __popcll(m & below);
                    if (pos >= off && pos < end) {
                        const int k = qq * 64 + bit;
                        const float a = lat_full[k];
                        const float b = lattice_mode == PERF_LATTICE_REPEATED ? add_rn(a, step) : lattice_single(t0_base, k + 1, step);
                        ts[pos] = a;
                        te[pos] = b;
                        ray_indices[pos] = r;
                        if (x01) sample_point_store(rays_o + 3 * r, rays_d + 3 * r, a, b, bb, x01, sel, pos);
                    }
                }
                run += __popcll(m);
            }
        }
    };
    // the rays that have samples, four at a time: a quarter wave each while all four write at most 16 samples (the tail of a two-phase
    // sampler, a thin shell), else one after the other with all 64 lanes
    for (uint64_t rays = __ballot(cnt_mine > 0); rays;) {
        int sq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sq[j] = -1;
            if (rays) { sq[j] = __ffsll((unsigned long long)rays) - 1; rays &= rays - 1; }
        }
        const int quarter = lane >> 4;
        const int s_mine = quarter == 0 ? sq[0] : (quarter == 1 ? sq[1] : (quarter == 2 ? sq[2] : sq[3]));
        const int32_t cnt_q = __shfl(cnt_mine, s_mine < 0 ? 0 : s_mine), off_q = __shfl(off_mine, s_mine < 0 ? 0 : s_mine);
        if (__ballot(s_mine >= 0 && cnt_q > 16) == 0ull) {
            if (s_mine >= 0) walk(std::integral_constant<int, 16>{}, r_base + s_mine, cnt_q, off_q, lane & 15);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (sq[j] >= 0)
                    walk(std::integral_constant<int, 64>{}, r_base + sq[j], __builtin_amdgcn_readlane(cnt_mine, sq[j]), __builtin_amdgcn_readlane(off_mine, sq[j]), lane);
        }
    }
}

// ---------------- exclusive scan of int32 (counts -> offsets) -----------------------------------
constexpr int kScanBlock = 1024;   // elements per block (256 threads x 4)

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int y = __shfl_up(v, off);
        if (lane >= off) v += y;
    }
    return v;
}

// block-wide exclusive scan of one int per thread (256 threads); returns exclusive value, total in *total
__device__ __forceinline__ int block_excl_scan(int v, int* lds4, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_incl_scan(v, lane);
    if (lane == 63) lds4[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w2 = 0; w2 < wave; ++w2) base += lds4[w2];
    *total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(256) void scan_block_sums_kernel(const int32_t* __restrict__ in, int64_t n, int64_t* __restrict__ sums) {
    __shared__ int lds4[4];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * 4;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (base + k < n) s += in[base + k];
    int total;
    block_excl_scan(s, lds4, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Second (and last) launch of the large scan: block b adds up the sums of the blocks before it itself (at most a few thousand
// 8-byte values from L2 -- a third launch that scans them cost 7.4 us, twice per 512x1024 frame), then scans its own 1024
// elements; the last block leaves the total.
// (Beyond kScanApplyMaxBlocks blocks -- more than 2 M elements -- the re-summing would grow quadratically: 8 M elements = 8,192 blocks =
//  33 M loads.  A middle launch then turns the block sums into exclusive prefixes once (scan_sums_kernel) and every block reads its own.)
constexpr int64_t kScanApplyMaxBlocks = 2048;
__global__ __launch_bounds__(1024) void scan_sums_kernel(int64_t* __restrict__ sums, int64_t nb) {
    __shared__ long long wave_tot[16];
    __shared__ long long carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t j = b0 + threadIdx.x;
        const long long v = j < nb ? sums[j] : 0;
        long long inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const long long t = __shfl_up(inc, off); if (lane >= off) inc += t; }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        long long before = carry_s;
        for (int w2 = 0; w2 < wave; ++w2) before += wave_tot[w2];
        if (j < nb) sums[j] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = before + inc;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void scan_apply_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n,
                                                         const int64_t* __restrict__ sums, int64_t* __restrict__ total_out,
                                                         int64_t bias, int64_t* __restrict__ total_biased, int sums_are_prefixes) {
    __shared__ int lds4[4];
    __shared__ long long pre4[4];
    long long before = 0;
    if (sums_are_prefixes) { if (threadIdx.x == 0) before = sums[blockIdx.x]; }
    else for (int64_t j = threadIdx.x; j < (int64_t)blockIdx.x; j += 256) before += sums[j];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off);
    if ((threadIdx.x & 63) == 0) pre4[threadIdx.x >> 6] = before;
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * 4;
    int v[4];
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
    int total;
    const int ex0 = block_excl_scan(s, lds4, &total);       // (its barriers order pre4 as well)
    const long long prefix = (pre4[0] + pre4[1]) + (pre4[2] + pre4[3]);
    int ex = ex0 + (int)prefix;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) out[base + k] = ex;
        ex += v[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *total_out = prefix + total;
        if (total_biased) *total_biased = prefix + total + bias;
    }
}

// n <= kScanSmall: ONE launch of ceil(n / 1024) workgroups.  Block b first sums every element BEFORE its segment itself
// (redundant, coalesced reads of at most 256 KiB from L2 -- far cheaper than a second launch or a cross-block handshake),
// then scans its own 1024 elements.  (The 8,192 per-ray counts of a training batch take 8 blocks; a single-workgroup
// scan of the 32,768 counts of an eval batch cost 27 us per call, 0.86 ms per 512x1024 frame.)
constexpr int kScanSmall = 65536;
__global__ __launch_bounds__(1024) void scan_small_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n,
                                                          int64_t* __restrict__ total_out, int64_t bias, int64_t* __restrict__ total_biased) {
    __shared__ long long wave_sum[16];
    __shared__ int wave_tot[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t seg_lo = (int64_t)blockIdx.x * 1024;
    // ---- sum of everything before the segment
    // (seg_lo is a multiple of 1024: 16-byte loads, four independent accumulators -- the loop is latency bound)
    long long s = 0;
    {
        const int4* in4 = reinterpret_cast<const int4*>(in);
        const int64_t n4 = seg_lo >> 2;
        long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int64_t i = threadIdx.x;
        if ((reinterpret_cast<uintptr_t>(in) & 15) == 0) {
            for (; i + 3 * 1024 < n4; i += 4 * 1024) {
                const int4 a = in4[i], b = in4[i + 1024], c = in4[i + 2048], d = in4[i + 3072];
                s0 += (long long)a.x + a.y + a.z + a.w; s1 += (long long)b.x + b.y + b.z + b.w;
                s2 += (long long)c.x + c.y + c.z + c.w; s3 += (long long)d.x + d.y + d.z + d.w;
            }
            for (; i < n4; i += 1024) { const int4 a = in4[i]; s0 += (long long)a.x + a.y + a.z + a.w; }
        } else {
            for (int64_t j = threadIdx.x; j < seg_lo; j += 1024) s0 += in[j];
        }
        s = (s0 + s1) + (s2 + s3);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) wave_sum[wave] = s;
    // ---- scan of the segment: wave scans + the 16 wave totals
    const int64_t i = seg_lo + threadIdx.x;
    const int v = (i < n) ? in[i] : 0;
    const int inc = wave_incl_scan(v, lane);
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    long long base = 0;
    int before = 0, seg_total = 0;
#pragma unroll
    for (int w2 = 0; w2 < 16; ++w2) { base += wave_sum[w2]; if (w2 < wave) before += wave_tot[w2]; seg_total += wave_tot[w2]; }
    if (i < n) out[i] = (int)base + before + inc - v;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *total_out = base + seg_total;
        if (total_biased) *total_biased = base + seg_total + bias;
    }
}

}  // namespace perf

using namespace perf;

static inline int chunk_words(int32_t max_steps) { return max_steps > 0 ? (max_steps + 63) / 64 : 0; }

// uint64 words per ray in the mask buffer: one mask word per 64-interval chunk plus the live-chunk words
extern "C" int64_t perf_occ_mask_words(int32_t max_steps) {
    const int mw = chunk_words(max_steps);
    return mw + (mw + 63) / 64;
}

extern "C" int64_t perf_occ_coarse_words(int32_t res) {
    if (res <= 0 || (res % 8) != 0) return 0;
    return coarse_words_of(res) + fine_words_of(res);           // the dilated 4^3-block grid, then the dilated 2^3-block grid
}

extern "C" int perf_occ_build_coarse(const uint32_t* occ_bits, int32_t res, uint32_t* coarse, void* stream) {
    PERF_REQUIRE(occ_bits && coarse && res > 0 && (res % 8) == 0, "perf_occ_build_coarse: res must be a positive multiple of 8");
    const int64_t words = perf_occ_coarse_words(res);
    hipError_t e = hipMemsetAsync(coarse, 0, words * sizeof(uint32_t), as_stream(stream));
    if (e != hipSuccess) { set_error("perf_occ_build_coarse: memset failed"); return PERF_E_LAUNCH; }
    const int cr = res / kCoarseBlock;
    hipLaunchKernelGGL(coarse_build_kernel, dim3((unsigned)div_up((int64_t)cr * cr * cr, 256)), dim3(256), 0, as_stream(stream),
                       occ_bits, (int)res, coarse);
    const int64_t fr = res / kFineBlock;
    hipLaunchKernelGGL(fine_build_kernel, dim3((unsigned)div_up(fr * fr * fr, 256)), dim3(256), 0, as_stream(stream),
                       occ_bits, (int)res, coarse + coarse_words_of(res));
    PERF_LAUNCH_CHECK("perf_occ_build_coarse");
    return PERF_OK;
}

static MarchParams march_params(const uint32_t* occ_coarse, int32_t res, const float* aabb, float far_plane, float step, int32_t max_steps,
                                int32_t lattice_mode) {
    MarchParams mp;
    for (int a = 0; a < 3; ++a) {
        mp.lo[a] = aabb[a]; mp.hi[a] = aabb[3 + a];
        mp.inv_ext[a] = 1.0f / (aabb[3 + a] - aabb[a]);
    }
    mp.far_plane = far_plane; mp.step = step; mp.res = res; mp.max_steps = max_steps; mp.lattice_mode = lattice_mode;
    mp.mask_words = chunk_words(max_steps);
    for (int a = 0; a < 3; ++a) mp.chunk_cells[a] = 64.0f * step * mp.inv_ext[a] * (float)res;
    mp.use_coarse = (occ_coarse != nullptr && (res % 8) == 0) ? 1 : 0;      // (+ the per-ray span test in the kernel)
    return mp;
}

static int march_count_launch(const float* rays_o, const float* rays_d, const float* t0, float t0_scale, float t0_base, int64_t n_rays,
                              const uint32_t* occ_bits, const uint32_t* occ_coarse, int32_t res, const float* aabb, float far_plane,
                              float step, int32_t max_steps, int32_t lattice_mode, const float* lattice_table, uint64_t* masks, int32_t* counts,
                              const HeadOut* head, void* stream) {
    PERF_REQUIRE(lattice_mode == PERF_LATTICE_SINGLE || lattice_mode == PERF_LATTICE_REPEATED, "bad lattice mode %d", (int)lattice_mode);
    PERF_REQUIRE(n_rays >= 0 && res > 0 && res <= 1024 && max_steps > 0 && step > 0.f, "perf_occ_march_count: bad arguments");
    if (n_rays == 0) return PERF_OK;
    PERF_REQUIRE(rays_o && rays_d && occ_bits && aabb && masks && counts, "NULL pointer");
    const MarchParams mp = march_params(occ_coarse, res, aabb, far_plane, step, max_steps, lattice_mode);
    SharedRuns sr;
    sr.n = 0;
    PERF_REQUIRE(!lattice_table || t0 == nullptr || lattice_mode == PERF_LATTICE_REPEATED, "per-ray lattice tables (t0 != NULL) exist for the repeated lattice only");
    if (lattice_mode == PERF_LATTICE_REPEATED && t0 == nullptr && !lattice_table) shared_runs_build(t0_base, step, mp.mask_words * 64 + 64, &sr);
    if (t0 == nullptr && lattice_table != nullptr && mp.mask_words <= 64 && n_rays >= kSharedMinRays && (!head || head->K <= kSharedHeadMax)) {      // (see march_count_shared_kernel)
        if (head)
            hipLaunchKernelGGL(march_count_shared_kernel<true>, dim3((unsigned)div_up(n_rays, 64)), dim3(64), 0, as_stream(stream), mp, rays_o, rays_d,
                               n_rays, occ_bits, occ_coarse, masks, counts, *head, t0_base, lattice_table);
        else
            hipLaunchKernelGGL(march_count_shared_kernel<false>, dim3((unsigned)div_up(n_rays, 64)), dim3(64), 0, as_stream(stream), mp, rays_o, rays_d,
                               n_rays, occ_bits, occ_coarse, masks, counts, HeadOut{}, t0_base, lattice_table);
        PERF_LAUNCH_CHECK("perf_occ_march_count");
        return PERF_OK;
    }
    if (head)
        hipLaunchKernelGGL(march_count_kernel<true>, dim3((unsigned)div_up(n_rays, 4)), dim3(256), 0, as_stream(stream), mp, rays_o,
                           rays_d, t0, n_rays, occ_bits, occ_coarse, masks, counts, *head, t0_scale, t0_base, sr, lattice_table);
    else
        hipLaunchKernelGGL(march_count_kernel<false>, dim3((unsigned)div_up(n_rays, 4)), dim3(256), 0, as_stream(stream), mp, rays_o,
                           rays_d, t0, n_rays, occ_bits, occ_coarse, masks, counts, HeadOut{}, t0_scale, t0_base, sr, lattice_table);
    PERF_LAUNCH_CHECK("perf_occ_march_count");
    return PERF_OK;
}

extern "C" int perf_occ_march_count(const float* rays_o, const float* rays_d, const float* t0, float t0_scale, float t0_base,
                                    int64_t n_rays, const uint32_t* occ_bits, const uint32_t* occ_coarse, int32_t res,
                                    const float* aabb, float far_plane, float step, int32_t max_steps, int32_t lattice_mode,
                                    const float* lattice_table, uint64_t* masks, int32_t* counts, void* stream) {
    return march_count_launch(rays_o, rays_d, t0, t0_scale, t0_base, n_rays, occ_bits, occ_coarse, res, aabb, far_plane, step, max_steps,
                              lattice_mode, lattice_table, masks, counts, nullptr, stream);
}

extern "C" int perf_occ_march_count_head(const float* rays_o, const float* rays_d, const float* t0, float t0_scale, float t0_base,
                                         int64_t n_rays, const uint32_t* occ_bits, const uint32_t* occ_coarse, int32_t res, const float* aabb,
                                         float far_plane, float step, int32_t max_steps, int32_t lattice_mode, const float* lattice_table,
                                         uint64_t* masks, int32_t* counts, int32_t head_k, int64_t* ray_indices, float* t_starts, float* t_ends, int32_t* packed_info,
                                         const float* points_aabb6, float* x01, uint8_t* sel, void* stream) {
    PERF_REQUIRE(head_k >= 1 && head_k <= 64, "perf_occ_march_count_head: head_k must be in [1, 64]");
    PERF_REQUIRE(n_rays == 0 || (ray_indices && t_starts && t_ends && packed_info && points_aabb6 && x01 && sel), "NULL pointer");
    PERF_REQUIRE(n_rays * (int64_t)head_k < ((int64_t)1 << 31), "perf_occ_march_count_head: n_rays * head_k exceeds int32 offsets");
    HeadOut ho;
    ho.K = head_k; ho.ri = ray_indices; ho.ts = t_starts; ho.te = t_ends; ho.packed = packed_info; ho.x01 = x01; ho.sel = sel;
    if (n_rays > 0) for (int a = 0; a < 3; ++a) { ho.bb.lo[a] = points_aabb6[a]; ho.bb.hi[a] = points_aabb6[3 + a]; }
    return march_count_launch(rays_o, rays_d, t0, t0_scale, t0_base, n_rays, occ_bits, occ_coarse, res, aabb, far_plane, step, max_steps,
                              lattice_mode, lattice_table, masks, counts, &ho, stream);
}

extern "C" int64_t perf_scan_workspace_bytes(int64_t n) { return (div_up(n > 0 ? n : 1, kScanBlock) + 1) * (int64_t)sizeof(int64_t); }

extern "C" int perf_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t* total, int64_t n, int64_t total_bias,
                                       int64_t* total_biased, void* workspace, int64_t workspace_bytes, void* stream) {
    PERF_REQUIRE(n >= 0 && total, "perf_exclusive_scan_i32: bad arguments");
    if (n == 0) {
        PERF_REQUIRE(!total_biased, "perf_exclusive_scan_i32: a biased total needs n > 0");
        hipError_t e = hipMemsetAsync(total, 0, sizeof(int64_t), as_stream(stream));
        if (e != hipSuccess) { set_error("memset failed"); return PERF_E_LAUNCH; }
        return PERF_OK;
    }
    PERF_REQUIRE(in && out && workspace, "NULL pointer");
    PERF_REQUIRE(workspace_bytes >= perf_scan_workspace_bytes(n), "scan workspace too small");
    PERF_REQUIRE(in != out, "perf_exclusive_scan_i32: in-place scan is not supported");
    if (n <= kScanSmall) {
        hipLaunchKernelGGL(scan_small_kernel, dim3((unsigned)div_up(n, 1024)), dim3(1024), 0, as_stream(stream), in, out, n, total, total_bias,
                           total_biased);
        PERF_LAUNCH_CHECK("perf_exclusive_scan_i32");
        return PERF_OK;
    }
    const int64_t nb = div_up(n, kScanBlock);
    int64_t* sums = (int64_t*)workspace;
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), in, n, sums);
    const int prefixes = nb > kScanApplyMaxBlocks ? 1 : 0;
    if (prefixes) hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, as_stream(stream), sums, nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), in, out, n, sums, total, total_bias,
                       total_biased, prefixes);
    PERF_LAUNCH_CHECK("perf_exclusive_scan_i32");
    return PERF_OK;
}

extern "C" int perf_occ_march_write(const float* t0, float t0_scale, float t0_base, int64_t n_rays, float step, int32_t max_steps,
                                    int32_t lattice_mode, const float* lattice_table, const uint64_t* masks,
                                    const int32_t* counts, const int32_t* offsets, int64_t capacity, int64_t* ray_indices,
                                    float* t_starts, float* t_ends, int32_t* packed_info, void* stream) {
    PERF_REQUIRE(n_rays >= 0 && max_steps > 0 && capacity >= 0, "perf_occ_march_write: bad arguments");
    if (n_rays == 0) return PERF_OK;
    PERF_REQUIRE(masks && counts && offsets && packed_info, "NULL pointer");
    PERF_REQUIRE(capacity == 0 || (ray_indices && t_starts && t_ends), "NULL sample arrays");
    SharedRuns sr;
    sr.n = 0;
    PERF_REQUIRE(!lattice_table || t0 == nullptr || lattice_mode == PERF_LATTICE_REPEATED, "per-ray lattice tables (t0 != NULL) exist for the repeated lattice only");
    if (lattice_mode == PERF_LATTICE_REPEATED && t0 == nullptr && !lattice_table) shared_runs_build(t0_base, step, chunk_words(max_steps) * 64 + 64, &sr);
    if (t0 == nullptr && lattice_table != nullptr && n_rays >= kSharedMinRays)        // (see march_write_shared_kernel)
        hipLaunchKernelGGL(march_write_shared_kernel, dim3((unsigned)div_up(n_rays, 256)), dim3(256), 0, as_stream(stream), n_rays, step,
                           (int32_t)chunk_words(max_steps), masks, counts, offsets, capacity, ray_indices, t_starts, t_ends, packed_info,
                           (const float*)nullptr, (const float*)nullptr, Aabb{}, (float*)nullptr, (uint8_t*)nullptr, 0, t0_base, (int)lattice_mode, lattice_table);
    else
    hipLaunchKernelGGL(march_write_kernel, dim3((unsigned)(n_rays / 4 >= 8192 ? div_up(n_rays, 16) : div_up(n_rays, 4))), dim3(256), 0, as_stream(stream), t0, n_rays,
                       step, (int32_t)chunk_words(max_steps), masks, counts, offsets, capacity, ray_indices, t_starts,
                       t_ends, packed_info, (const float*)nullptr, (const float*)nullptr, Aabb{}, (float*)nullptr, (uint8_t*)nullptr, 0, t0_scale, t0_base, (int)lattice_mode, sr, lattice_table);
    PERF_LAUNCH_CHECK("perf_occ_march_write");
    return PERF_OK;
}

extern "C" int perf_occ_march_write_points(const float* t0, float t0_scale, float t0_base, int64_t n_rays, float step, int32_t max_steps,
                                           int32_t lattice_mode, const float* lattice_table, const uint64_t* masks,
                                           const int32_t* counts, const int32_t* offsets, int64_t capacity, int64_t* ray_indices,
                                           float* t_starts, float* t_ends, int32_t* packed_info, const float* rays_o,
                                           const float* rays_d, const float* aabb6, float* x01, uint8_t* sel, int32_t rank_lo,
                                           void* stream) {
    PERF_REQUIRE(n_rays >= 0 && max_steps > 0 && capacity >= 0 && rank_lo >= 0, "perf_occ_march_write_points: bad arguments");
    if (n_rays == 0) return PERF_OK;
    PERF_REQUIRE(masks && counts && offsets && packed_info && rays_o && rays_d && aabb6, "NULL pointer");
    PERF_REQUIRE(capacity == 0 || (ray_indices && t_starts && t_ends && x01), "NULL sample arrays");
    Aabb bb;
    for (int k = 0; k < 3; ++k) { bb.lo[k] = aabb6[k]; bb.hi[k] = aabb6[3 + k]; }
    SharedRuns sr;
    sr.n = 0;
    PERF_REQUIRE(!lattice_table || t0 == nullptr || lattice_mode == PERF_LATTICE_REPEATED, "per-ray lattice tables (t0 != NULL) exist for the repeated lattice only");
    if (lattice_mode == PERF_LATTICE_REPEATED && t0 == nullptr && !lattice_table) shared_runs_build(t0_base, step, chunk_words(max_steps) * 64 + 64, &sr);
    if (t0 == nullptr && lattice_table != nullptr && n_rays >= kSharedMinRays)        // (see march_write_shared_kernel)
        hipLaunchKernelGGL(march_write_shared_kernel, dim3((unsigned)div_up(n_rays, 256)), dim3(256), 0, as_stream(stream), n_rays, step,
                           (int32_t)chunk_words(max_steps), masks, counts, offsets, capacity, ray_indices, t_starts, t_ends, packed_info,
                           rays_o, rays_d, bb, x01, sel, rank_lo, t0_base, (int)lattice_mode, lattice_table);
    else
    hipLaunchKernelGGL(march_write_kernel, dim3((unsigned)(n_rays / 4 >= 8192 ? div_up(n_rays, 16) : div_up(n_rays, 4))), dim3(256), 0, as_stream(stream), t0, n_rays,
                       step, (int32_t)chunk_words(max_steps), masks, counts, offsets, capacity, ray_indices, t_starts,
                       t_ends, packed_info, rays_o, rays_d, bb, x01, sel, rank_lo, t0_scale, t0_base, (int)lattice_mode, sr, lattice_table);
    PERF_LAUNCH_CHECK("perf_occ_march_write_points");
    return PERF_OK;
}

// ---- per-ray tables of runs: one LANE per ray ------------------------------------------------------------------------------
namespace perf {

__global__ __launch_bounds__(64) void lattice_runs_kernel(const float* __restrict__ t0s, float t0_scale, float t0_base, int64_t n_rays,
                                                          float step, int32_t k_need, int32_t* __restrict__ rows) {
    lattice_runs_row((int64_t)blockIdx.x * 64 + threadIdx.x, t0s, t0_scale, t0_base, n_rays, step, k_need, rows);
}
}  // namespace perf

extern "C" int64_t perf_occ_lattice_runs_len(int64_t n_rays) { return (n_rays > 0 ? n_rays : 0) * (int64_t)kRunsStride; }

extern "C" int perf_occ_lattice_runs(const float* t0, float t0_scale, float t0_base, int64_t n_rays, float step, int32_t max_steps,
                                     int32_t* runs, void* stream) {
    PERF_REQUIRE(n_rays >= 0 && max_steps > 0 && step > 0.f, "perf_occ_lattice_runs: bad arguments");
    if (n_rays == 0) return PERF_OK;
    PERF_REQUIRE(t0 && runs, "NULL pointer");
    hipLaunchKernelGGL(perf::lattice_runs_kernel, dim3((unsigned)div_up(n_rays, 64)), dim3(64), 0, as_stream(stream), t0, t0_scale, t0_base, n_rays,
                       step, (int32_t)(chunk_words(max_steps) * 64 + 64), runs);
    PERF_LAUNCH_CHECK("perf_occ_lattice_runs");
    return PERF_OK;
}

// t_k, k = 0 .. n-1, of the lattice that starts at t0 -- for launches whose rays all share it (eval renders: no stratified jitter).
// The marching entry points take the table as `lattice_table`: a lattice point is then ONE load instead of a walk (repeated
// addition) -- a 512x1024 eval frame marches 0.5 M rays on the same 3,000 points.
namespace perf {
__global__ __launch_bounds__(256) void lattice_table_kernel(float t0, float step, int32_t n, int mode, float* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = lattice(t0, k, step, mode);
}
}  // namespace perf

extern "C" int64_t perf_occ_lattice_table_len(int32_t max_steps) { return (int64_t)chunk_words(max_steps) * 64 + 66; }

extern "C" int perf_occ_lattice_table(float t0, float step, int32_t max_steps, int32_t lattice_mode, float* table, void* stream) {
    PERF_REQUIRE(table && max_steps > 0 && step > 0.f, "perf_occ_lattice_table: bad arguments");
    PERF_REQUIRE(lattice_mode == PERF_LATTICE_SINGLE || lattice_mode == PERF_LATTICE_REPEATED, "bad lattice mode %d", (int)lattice_mode);
    const int32_t n = (int32_t)perf_occ_lattice_table_len(max_steps);
    hipLaunchKernelGGL(perf::lattice_table_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, as_stream(stream), t0, step, n,
                       (int)lattice_mode, table);
    PERF_LAUNCH_CHECK("perf_occ_lattice_table");
    return PERF_OK;
}


// ---- step riders (include/perf_hip_riders.h): the argument blocks checked and turned into the jobs the host launches carry -------------
extern "C" int perf_riders_version(void) { return PERF_RIDERS_ABI_VERSION; }
extern "C" int64_t perf_sizeof_rider_draw(void) { return (int64_t)sizeof(perf_rider_draw); }
extern "C" int64_t perf_sizeof_rider_count(void) { return (int64_t)sizeof(perf_rider_count); }
extern "C" int64_t perf_sizeof_rider_write(void) { return (int64_t)sizeof(perf_rider_write); }

int perf_internal_rider_draw_job(const perf_rider_draw* a, RiderDrawJob* job) {
    job->n_blocks = 0;
    if (!a) return PERF_OK;
    // (perf_draw_train_batch's and perf_occ_lattice_runs's own checks)
    PERF_REQUIRE(a->counter_dev && a->ticket, "perf_rider_draw: NULL counter / ticket");
    PERF_REQUIRE(a->pool_hi > a->pool_lo && a->pool_lo >= 0 && a->pool_hi - a->pool_lo < ((int64_t)1 << 32), "perf_rider_draw: bad pool range");
    PERF_REQUIRE(a->n_local > 0 && a->first_global >= 0 && a->n_local <= PERF_RIDER_MAX_RAYS, "perf_rider_draw: bad batch");
    PERF_REQUIRE((!a->o || a->o_all) && (!a->d || a->d_all) && (!a->color || a->color_all) && (!a->dist || a->dist_all) && (!a->normal || a->normal_all),
                 "perf_rider_draw: output without source");
    PERF_REQUIRE(a->jitter && a->runs && a->max_steps > 0 && a->step > 0.f, "perf_rider_draw: the lattice tables need jitter, runs, max_steps > 0 and step > 0");
    PERF_REQUIRE((a->marched_live != nullptr) == (a->marched_keep != nullptr), "perf_rider_draw: marched_live and marched_keep go together");
    job->a = *a;
    job->k_need = (int32_t)(chunk_words(a->max_steps) * 64 + 64);
    job->n_blocks = (int32_t)div_up(a->n_local, PERF_RIDER_DRAW_RAYS);
    return PERF_OK;
}

int perf_internal_rider_count_job(const perf_rider_count* a, RiderCountJob* job) {
    job->n_blocks = 0;
    if (!a) return PERF_OK;
    PERF_REQUIRE(a->n_rays > 0 && a->n_rays <= PERF_RIDER_MAX_RAYS && a->res > 0 && a->res <= 1024 && a->max_steps > 0 && a->step > 0.f,
                 "perf_rider_count: bad arguments");
    PERF_REQUIRE(a->rays_o && a->rays_d && a->occ_bits && a->masks && a->counts, "perf_rider_count: NULL pointer");
    PERF_REQUIRE(a->t0 && a->runs, "perf_rider_count: per-ray origins (t0) and their tables of runs are required");
    job->mp = march_params(a->occ_coarse, a->res, a->aabb, a->far_plane, a->step, a->max_steps, PERF_LATTICE_REPEATED);
    job->ro = a->rays_o; job->rd = a->rays_d; job->t0s = a->t0; job->t0_scale = a->t0_scale; job->t0_base = a->t0_base; job->n_rays = a->n_rays;
    job->bits = a->occ_bits; job->coarse = a->occ_coarse; job->runs = a->runs; job->masks = a->masks; job->counts = a->counts;
    job->n_blocks = (int32_t)div_up(a->n_rays, PERF_RIDER_MARCH_RAYS);
    return PERF_OK;
}

int perf_internal_rider_write_job(const perf_rider_write* a, RiderWriteJob* job) {
    job->n_blocks = 0;
    if (!a) return PERF_OK;
    PERF_REQUIRE(a->n_rays > 0 && a->n_rays <= PERF_RIDER_MAX_RAYS && a->max_steps > 0 && a->capacity >= 0 && a->step > 0.f, "perf_rider_write: bad arguments");
    PERF_REQUIRE(a->masks && a->counts && a->offsets && a->total && a->packed_info && a->rays_o && a->rays_d, "perf_rider_write: NULL pointer");
    PERF_REQUIRE(a->t0 && a->runs, "perf_rider_write: per-ray origins (t0) and their tables of runs are required");
    PERF_REQUIRE(a->capacity == 0 || (a->ray_indices && a->t_starts && a->t_ends && a->x01 && a->sel), "perf_rider_write: NULL sample arrays");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(a->counts) & 15) == 0, "perf_rider_write: counts must be 16-byte aligned");
    job->a = *a;
    for (int k = 0; k < 3; ++k) { job->bb.lo[k] = a->points_aabb[k]; job->bb.hi[k] = a->points_aabb[3 + k]; }
    job->mask_words = (int32_t)chunk_words(a->max_steps);
    job->n_blocks = (int32_t)div_up(a->n_rays, PERF_RIDER_MARCH_RAYS);
    return PERF_OK;
}
