// Device side of the occupancy-grid marching (march.hip): lattice arithmetic, the per-ray tables of runs and the bodies of the
// counting and the write pass as device functions of a 256-thread workgroup, so that the stand-alone kernels and the blocks that
// ride in another launch (step_riders_device.hpp) run ONE body -- the same bits either way.
#pragma once
#include "common.hpp"

namespace perf {

struct MarchParams {
    float lo[3], inv_ext[3];
    float hi[3];
    float far_plane, step;
    int32_t res, max_steps, mask_words;
    int32_t lattice_mode;    // PERF_LATTICE_*
    int32_t use_coarse;      // 1: skip 64-interval chunks whose midpoint lies in an empty DILATED block (kCoarseBlock^3 cells)
    float chunk_cells[3];    // fine cells a 64-interval chunk spans per unit of |d| along each axis (64 step res / extent)
};

// Coarse skip grid: bit b of `coarse` is set iff any fine cell in the 3x3x3 neighbourhood of B^3-block b is occupied
// (B = kCoarseBlock).  A chunk of 64 lattice intervals spans at most `span` fine cells; when span/2 + 1.5 <= B every
// midpoint of the chunk lies within one block of the block that holds the chunk's centre, so an empty dilated block proves
// the chunk empty (conservative: results are identical to the exhaustive test).  B = 4: at PeRF's step (5e-4, 4.1 cells per
// chunk) the condition holds with the smallest power of two, and a thin occupied shell keeps 3 blocks = 12 cells = ~3
// chunks of a ray alive instead of the ~6 that 8^3 blocks kept -- phase B of march_count is what a frame pays for.
constexpr int kCoarseShift = 2;
constexpr int kCoarseBlock = 1 << kCoarseShift;
// Fine skip grid, behind the coarse one in the same buffer (perf_occ_coarse_words counts both): bit b is set iff any fine cell in
// the 3x3x3 neighbourhood of the 2^3-block b is occupied.  A chunk that the coarse test lets through is tested again at TWO of
// its lattice points (k0 + 16, k0 + 48): every interval midpoint of the chunk lies within 16.5 intervals of one of them, i.e.
// within 0.258 span cells per axis -- while that (+ half a cell of slack) stays below the block size 2, the midpoint's block is the
// test point's block or a neighbour of it, so two empty dilated blocks prove the chunk empty (conservative: masks and counts are
// what the exhaustive test gives; the bit-exact marching tests run through it).  Around a thin occupied shell the coarse grid keeps
// 12 + 4.1 cells = ~4-5 chunks of a ray alive, the fine one 6 + 4.1 = ~2.5.
constexpr int kFineShift = 1;
constexpr int kFineBlock = 1 << kFineShift;
__host__ __device__ __forceinline__ int64_t coarse_words_of(int res) { const int64_t cr = res >> kCoarseShift; return (cr * cr * cr + 31) / 32; }
__host__ __device__ __forceinline__ int64_t fine_words_of(int res) { const int64_t fr = res >> kFineShift; return (fr * fr * fr + 31) / 32; }

// the fine block of a point on the ray (same position arithmetic as the cell look-ups)
__device__ __forceinline__ uint32_t fine_block_at(const MarchParams& mp, const float o[3], const float d[3], float t, float rf, int fr) {
    int cb[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = add_rn(o[a], mul_rn(d[a], t));
        const float u = mul_rn(mul_rn(sub_rn(p, mp.lo[a]), mp.inv_ext[a]), rf);
        cb[a] = ((int)fminf(fmaxf(floorf(u), 0.0f), rf - 1.0f)) >> kFineShift;
    }
    return (uint32_t)((cb[0] * fr + cb[1]) * fr + cb[2]);
}

__device__ __forceinline__ float lattice_single(float t0, int k, float step) { return add_rn(t0, mul_rn((float)k, step)); }

// PERF_LATTICE_REPEATED: t_0 = t0, t_{j+1} = fl(t_j + step) -- the lattice a marcher that ADVANCES by `t += dt` produces
// (nerfacc's traverse_grids, as far as it can be read without the package: oracle/perf_oracle.py header).  Evaluated for an
// arbitrary k without k additions: inside one binade consecutive floats have consecutive bit patterns, and from the second
// in-binade addition on every addition moves by the same number of ulps (round-to-nearest-even of step / ulp: a tie lands
// on an even mantissa once and then stays even) -- so the walk jumps binade by binade with two real additions each.
// floor(n / d) for n < 2^24, d >= 1: the reciprocal estimate is off by at most one (the compiler's generic 32-bit division is
// ~4x the instructions, and the walk below divides once per binade)
__device__ __forceinline__ uint32_t div_u24(uint32_t n, uint32_t d) {
    uint32_t q = (uint32_t)((float)n * __frcp_rn((float)d));
    const uint32_t p = q * d;
    if (p > n) --q;                                              // (estimate one too large)
    else if (n - p >= d) ++q;                                    // (one too small)
    return q;
}

__device__ __forceinline__ float lattice(float t0, int k, float step, int mode);

__device__ __forceinline__ float lattice_repeated(float t0, int k, float step) {
    float t = t0;
    int left = k;
    while (left > 0) {
        const float t1 = add_rn(t, step);
        if (--left == 0) return t1;
        if ((__float_as_uint(t1) >> 23) != (__float_as_uint(t) >> 23)) { t = t1; continue; }   // entered a binade: one more real step first
        const float t2 = add_rn(t1, step);
        if (--left == 0) return t2;
        const uint32_t b1 = __float_as_uint(t1), b2 = __float_as_uint(t2);
        if ((b2 >> 23) != (b1 >> 23)) { t = t2; continue; }
        const uint32_t d = b2 - b1;                              // ulps per step from here to the end of the binade
        if (d == 0u) return t2;                                  // (step below half an ulp: the lattice is stuck)
        const uint32_t top = (b2 & 0xff800000u) + 0x00800000u;   // first bit pattern of the next binade
        uint32_t j = div_u24(top - 1u - b2, d);                  // further additions that stay inside
        if (j > (uint32_t)left) j = (uint32_t)left;
        t = __uint_as_float(b2 + j * d);
        left -= (int)j;
    }
    return t;
}

// The same walk, ONCE per ray, as a table of runs: run i covers lattice indices [ks[i], ks[i+1]) and holds
// t_k = bits(bs[i] + (k - ks[i]) * dd[i]) -- inside a binade consecutive lattice points are equidistant bit patterns.
// march_count_kernel evaluates the lattice at 3 indices per chunk in phase A and once per lane and live chunk in phase B,
// i.e. thousands of per-lane walks per ray at PeRF's 3,000 steps (measured: the kernel went from 13 to 85 us per 8,192
// rays when the repeated lattice became the default); with the table a ray is walked once -- on values that are uniform
// over the wave (the float additions run on the vector unit, everything else on the scalar unit) -- and an evaluation is
// a binary search over <= kMaxRuns run starts in LDS.  Returns the number of runs, or -1 when the table does not reach
// index k_need (more binades than the table holds: the caller falls back to the per-lane walk).
constexpr int kMaxRuns = 64;

// (the walk runs on values that are uniform over the wave: the float additions go through the vector unit and come back with
//  readfirstlane, everything else stays on the scalar unit; lane 0 stores.  Letting lanes 0..3 of one wave walk the block's
//  four rays and synchronising the block measured SLOWER: 26.9 vs 20.6 us per 8,192 rays -- the other waves wait out the
//  walk's latency)
// UNIFORM: one ray per WAVE (values uniform over the wave, kept on the scalar unit through readfirstlane; lane 0 stores);
// otherwise one ray per LANE (lattice_runs_kernel) -- the same arithmetic either way, so the tables are identical.
template <bool UNIFORM>
__device__ __forceinline__ int lattice_runs_build(float t0, float step, int k_need, int32_t* __restrict__ ks, uint32_t* __restrict__ bs,
                                                  uint32_t* __restrict__ dd, bool writer) {
    int n = 0;
    auto emit = [&](int k, uint32_t b, uint32_t d) {
        if (writer) { ks[n] = k; bs[n] = b; dd[n] = d; }
        ++n;
    };
    auto uni = [](uint32_t v) { return UNIFORM ? (uint32_t)__builtin_amdgcn_readfirstlane((int)v) : v; };
    uint32_t tb = uni(__float_as_uint(t0));
    emit(0, tb, 0u);
    int K = 0;
    while (K < k_need) {
        if (n + 2 > kMaxRuns) return -1;
        const uint32_t b1 = uni(__float_as_uint(add_rn(__uint_as_float(tb), step)));
        if ((b1 >> 23) != (tb >> 23)) { emit(K + 1, b1, 0u); tb = b1; K += 1; continue; }    // entered a binade: one more real step first
        const uint32_t b2 = uni(__float_as_uint(add_rn(__uint_as_float(b1), step)));
        if ((b2 >> 23) != (b1 >> 23)) { emit(K + 1, b1, 0u); emit(K + 2, b2, 0u); tb = b2; K += 2; continue; }
        const uint32_t d = b2 - b1;
        emit(K + 1, b1, d);                                      // t_{K+1}, t_{K+2}, ... equidistant to the end of the binade
        if (d == 0u) return n;                                   // (step below half an ulp: the lattice is stuck at t_{K+1} for good)
        const uint32_t top = (b2 & 0xff800000u) + 0x00800000u;
        const uint32_t j = uni(div_u24(top - 1u - b2, d));
        tb = b2 + j * d;
        K += 2 + (int)j;
    }
    return n;
}

// Per-ray tables in device memory (perf_occ_lattice_runs): row r = [n | ks[kMaxRuns] | bs[kMaxRuns] | dd[kMaxRuns]] of
// kRunsStride 32-bit words (n = -1: the table did not fit, walk per lane).  The uniform build above costs a whole WAVE per ray --
// ~840 dependent vector instructions on uniform values, x 8,192 rays x 4 cycles each: 13 of the 27 us march_count took on a
// jittered training batch -- the kernel below gives every ray a LANE instead (128 waves for 8,192 rays).
constexpr int kRunsStride = 3 * kMaxRuns + 4;

// The table of a launch whose rays all start their lattice at the same t0 (eval renders: no stratified jitter): built ONCE
// on the host with the same IEEE single-precision additions and handed to the kernels as an argument.
struct SharedRuns {
    int32_t n;                    // 0: none (per-ray origins, or the single-rounding lattice); -1 cannot happen (the host falls back to 0)
    int32_t ks[kMaxRuns];
    uint32_t bs[kMaxRuns], dd[kMaxRuns];
};

__device__ __forceinline__ float lattice(float t0, int k, float step, int mode) {
    return mode == PERF_LATTICE_REPEATED ? lattice_repeated(t0, k, step) : lattice_single(t0, k, step);
}

struct LatticeRuns {
    int n;                       // > 0: table; <= 0: evaluate directly (single lattice, or a table that did not fit)
    const int32_t* ks; const uint32_t* bs; const uint32_t* dd;
    float t0, step; int mode;
    const float* full;           // != NULL: t_k for every k of the launch (all rays on one lattice, perf_occ_lattice_table): one load
    __device__ __forceinline__ int find(int k) const {           // last run that starts at or before k
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (ks[mid] <= k) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
    __device__ __forceinline__ float at(int r, int k) const { return __uint_as_float(bs[r] + (uint32_t)(k - ks[r]) * dd[r]); }
    __device__ __forceinline__ float operator()(int k) const {
        if (full) return full[k];
        if (n <= 0) return lattice(t0, k, step, mode);
        return at(find(k), k);
    }
    // a little further along the lattice than run r reaches: the next runs are tried before a search
    __device__ __forceinline__ float after(int& r, int k) const {
        if (full) return full[k];
        if (n <= 0) return lattice(t0, k, step, mode);
        while (r + 1 < n && ks[r + 1] <= k) ++r;
        return at(r, k);
    }
};

// t_k from a ray's row of the per-ray tables (device memory, L2 resident): binary search over the run starts
__device__ __forceinline__ float runs_row_at(const int32_t* __restrict__ row, int k, float t0, float step) {
    const int n = row[0];
    if (n <= 0) return lattice_repeated(t0, k, step);
    const int32_t* ks = row + 1;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ks[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return __uint_as_float((uint32_t)row[1 + kMaxRuns + lo] + (uint32_t)(k - ks[lo]) * (uint32_t)row[1 + 2 * kMaxRuns + lo]);
}

// Lattice origin of ray r.  t0s == NULL: t0_base (the near plane).  t0_scale == 0: t0s[r] as given.  Otherwise t0s holds the
// stratified draw u in [0,1) and the origin is fl(u * t0_scale) (+ t0_base when that is not 0) -- the two torch ops of
// OccGridEstimator.sampling (near_plane + u * render_step_size), formed here so that no separate launch is needed.
__device__ __forceinline__ float lattice_origin(const float* __restrict__ t0s, int64_t r, float t0_scale, float t0_base) {
    if (!t0s) return t0_base;
    float t = t0s[r];
    if (t0_scale != 0.f) {
        t = mul_rn(t, t0_scale);
        if (t0_base != 0.f) t = add_rn(t, t0_base);
    }
    return t;
}

// Per-ray record in the mask buffer: [live words | chunk masks]: bit q of the live words says chunk q (lattice
// intervals 64q..64q+63) may hold samples; only live chunks have their mask word written (and later read).
__device__ __forceinline__ int n_live_words(int mask_words) { return (mask_words + 63) >> 6; }

// HEAD: the first `K` samples of every ray (the head of the two-phase sampler) are written right here, to rows r*K .. r*K+K-1
// of arrays of n_rays*K rows (rows beyond a ray's count are padded with sel = 0) -- what used to take a count clamp, a scan
// over the rays and a pass of march_write_kernel.  Same values as that pass writes (lattice + sample_point_store).
struct HeadOut {
    int32_t K;
    int64_t* ri; float* ts; float* te; int32_t* packed;
    float* x01; uint8_t* sel;
    Aabb bb;
};

// The counting pass of workgroup `block` (256 threads: four rays, a wave each) -- march_count_kernel is this body.
template <bool HEAD>
__device__ __forceinline__ void march_count_body(int block, const MarchParams& mp, const float* __restrict__ ro,
                                                 const float* __restrict__ rd, const float* __restrict__ t0s,
                                                 int64_t n_rays, const uint32_t* __restrict__ bits,
                                                 const uint32_t* __restrict__ coarse,
                                                 uint64_t* __restrict__ masks, int32_t* __restrict__ counts, const HeadOut& ho,
                                                 float t0_scale, float t0_base, const SharedRuns& sr, const float* __restrict__ lat_full) {
    const int lane = threadIdx.x & 63;
    // (the ray index is wave uniform: saying so turns the loads of the ray's origin, direction and lattice origin into
    //  scalar loads -- seven vector-memory instructions per ray less; the kernel is bound by VMEM issue, not by bytes)
    const int64_t r = (int64_t)block * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // repeated-addition lattice: the ray's walk as a table of runs in LDS -- ONE table for the block when all rays start at the
    // same t0 (built on the host), else every wave walks its own ray
    __shared__ int32_t s_ks[4][kMaxRuns];
    __shared__ uint32_t s_bs[4][kMaxRuns], s_dd[4][kMaxRuns];
    __shared__ int32_t s_head[HEAD ? 4 : 1][64];       // HEAD: lattice indices of the ray's first K samples (written after the chunk loop)
    if (mp.lattice_mode == PERF_LATTICE_REPEATED && sr.n > 0) {
        if ((int)threadIdx.x < sr.n) { s_ks[0][threadIdx.x] = sr.ks[threadIdx.x]; s_bs[0][threadIdx.x] = sr.bs[threadIdx.x]; s_dd[0][threadIdx.x] = sr.dd[threadIdx.x]; }
        __syncthreads();
    }
    if (r >= n_rays) return;
    const float o[3] = {ro[3 * r], ro[3 * r + 1], ro[3 * r + 2]};
    const float d[3] = {rd[3 * r], rd[3 * r + 1], rd[3 * r + 2]};
    const float t0 = lattice_origin(t0s, r, t0_scale, t0_base);
    // slab test (fminf/fmaxf drop NaNs like np.fmin/np.fmax)
    float tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float inv = __fdiv_rn(1.0f, d[a]);
        const float t1 = mul_rn(sub_rn(mp.lo[a], o[a]), inv), t2 = mul_rn(sub_rn(mp.hi[a], o[a]), inv);
        const float l = fminf(t1, t2), h = fmaxf(t1, t2);
        tmin = (a == 0) ? l : fmaxf(tmin, l);
        tmax = (a == 0) ? h : fminf(tmax, h);
    }
    const float lo = fmaxf(tmin, t0), hi = fminf(tmax, mp.far_plane);
    const int wv = threadIdx.x >> 6;
    const int tab = sr.n > 0 ? 0 : wv;
    LatticeRuns lat;
    lat.n = 0;
    lat.ks = s_ks[tab]; lat.bs = s_bs[tab]; lat.dd = s_dd[tab]; lat.t0 = t0; lat.step = mp.step; lat.mode = mp.lattice_mode;
    // per-ray origins with a table argument: the rows of perf_occ_lattice_runs (not a shared t_k array)
    const int32_t* ray_row = (t0s && lat_full) ? reinterpret_cast<const int32_t*>(lat_full) + r * (int64_t)kRunsStride : nullptr;
    lat.full = ray_row ? nullptr : lat_full;
    if (ray_row) {
        if (mp.lattice_mode == PERF_LATTICE_REPEATED) {
            s_ks[wv][lane] = ray_row[1 + lane]; s_bs[wv][lane] = (uint32_t)ray_row[1 + kMaxRuns + lane]; s_dd[wv][lane] = (uint32_t)ray_row[1 + 2 * kMaxRuns + lane];
            lat.n = ray_row[0];
            __builtin_amdgcn_wave_barrier();
        }
    } else if (mp.lattice_mode == PERF_LATTICE_REPEATED && !lat_full) {
        if (sr.n > 0) lat.n = sr.n;
        else {
            lat.n = lattice_runs_build<true>(t0, mp.step, mp.mask_words * 64 + 64, s_ks[wv], s_bs[wv], s_dd[wv], lane == 0);
            __builtin_amdgcn_wave_barrier();
        }
    }
    // the coarse skip is only valid while a chunk spans few enough fine cells (see coarse_build_kernel): checked per ray
    // with its own direction, so unnormalised directions fall back to the exhaustive test instead of skipping cells
    float span_cells = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) span_cells = fmaxf(span_cells, fabsf(d[a]) * mp.chunk_cells[a]);
    const bool use_coarse = mp.use_coarse && (span_cells * 0.5f + 1.5f <= (float)kCoarseBlock);
    const bool use_fine = use_coarse && (span_cells * (16.5f / 64.0f) + 0.5f <= (float)kFineBlock);
    int32_t count = 0;
    const int res = mp.res;
    const float rf = (float)res;
    const uint32_t* fine = coarse ? coarse + coarse_words_of(res) : nullptr;
    const int nlw = n_live_words(mp.mask_words);
    uint64_t* rec = masks + r * (int64_t)(mp.mask_words + nlw);
    for (int g = 0; g < nlw; ++g) {
        // ---- phase A: lane q decides whether chunk 64g+q can hold a sample at all (range + dilated coarse grid):
        //      one ballot replaces up to 64 sequential chunk visits (what nerfacc's DDA skips cell by cell)
        const int q = g * 64 + lane;
        bool maybe = false;
        int run_at_chunk = 0;           // table of runs: the run that holds this lane's chunk start (phase B starts its look-ups there)
        if (q < mp.mask_words) {
            const int k0 = q * 64;
            int run = (lat.n > 0 && !lat.full) ? lat.find(k0) : 0;
            run_at_chunk = run;
            const float t_first = (lat.n > 0 && !lat.full) ? lat.at(run, k0) : lat(k0);
            const float t_mid = lat.after(run, k0 + 32), t_last = lat.after(run, k0 + 64);
            maybe = !(t_first > hi) && !(t_last < lo);
            if (maybe && use_coarse) {
                const float tc = t_mid;
                const int cr = res >> kCoarseShift;
                int cb[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float p = add_rn(o[a], mul_rn(d[a], tc));
                    const float u = mul_rn(mul_rn(sub_rn(p, mp.lo[a]), mp.inv_ext[a]), rf);
                    cb[a] = ((int)fminf(fmaxf(floorf(u), 0.0f), rf - 1.0f)) >> kCoarseShift;
                }
                const uint32_t bi = (uint32_t)((cb[0] * cr + cb[1]) * cr + cb[2]);
                maybe = (coarse[bi >> 5] >> (bi & 31)) & 1u;
                if (maybe && use_fine) {
                    const int fr = res >> kFineShift;
                    int run2 = run_at_chunk;                                 // (`run` has moved on to k0 + 64)
                    const uint32_t f1 = fine_block_at(mp, o, d, lat.after(run2, k0 + 16), rf, fr);
                    const uint32_t f3 = fine_block_at(mp, o, d, lat.after(run2, k0 + 48), rf, fr);
                    maybe = (((fine[f1 >> 5] >> (f1 & 31)) | (fine[f3 >> 5] >> (f3 & 31))) & 1u) != 0u;
                }
            }
        }
        uint64_t live = __ballot(maybe);
        uint64_t kept = 0;        // chunks that really hold samples
        // ---- phase B: the 64 lattice intervals of every surviving chunk, one per lane.  Four chunks per round: their
        //      occupancy words are independent gathers, issued together instead of one L2 latency after the other
        //      (a ray crosses ~5 live chunks around a surface: the dilated coarse grid is generous)
        for (uint64_t todo = live; todo;) {
            int qs[4]; uint32_t cis[4]; bool in_range[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                qs[u] = -1; cis[u] = 0u; in_range[u] = false;
                if (todo) {
                    qs[u] = g * 64 + (__ffsll((unsigned long long)todo) - 1);
                    todo &= todo - 1;
                    const int k = qs[u] * 64 + lane;
                    // (the chunk is wave uniform: ONE lane's run index for all -- v_readlane, whatever the exec mask)
                    int r_lo = __builtin_amdgcn_readlane(run_at_chunk, qs[u] & 63);
                    if (k < mp.max_steps) {
                        float ta;
                        // table of runs: look-ups start at the run of the chunk's first index instead of a binary search per lane (the
                        // ray's FIRST chunk crosses a dozen runs -- one or two per binade from 2^-11 up -- and keeps the search)
                        if (lat.n > 0 && !lat.full && qs[u] != 0) ta = lat.after(r_lo, k);
                        else ta = lat(k);
                        const float tb = mp.lattice_mode == PERF_LATTICE_REPEATED ? add_rn(ta, mp.step) : lattice_single(t0, k + 1, mp.step);
                        const float mid = mul_rn(add_rn(ta, tb), 0.5f);
                        if (mid >= lo && mid <= hi) {
                            int cell[3];
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                const float p = add_rn(o[a], mul_rn(d[a], mid));
                                const float uu = mul_rn(mul_rn(sub_rn(p, mp.lo[a]), mp.inv_ext[a]), rf);
                                cell[a] = (int)fminf(fmaxf(floorf(uu), 0.0f), rf - 1.0f);
                            }
                            cis[u] = (uint32_t)((cell[0] * res + cell[1]) * res + cell[2]);
                            in_range[u] = true;
                        }
                    }
                }
            }
            uint32_t words[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) words[u] = in_range[u] ? bits[cis[u] >> 5] : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (qs[u] < 0) continue;                 // (wave uniform)
                const bool mine = in_range[u] && ((words[u] >> (cis[u] & 31)) & 1u);
                const uint64_t m = __ballot(mine);
                if (m) {
                    kept |= 1ull << (qs[u] & 63);
                    if (lane == 0) rec[nlw + qs[u]] = m;
                    if (HEAD && count < ho.K && mine) {         // (chunks arrive in t order: `count` = samples before this chunk)
                        const int rank = count + __popcll(m & ((1ull << lane) - 1ull));
                        if (rank < ho.K) s_head[wv][rank] = qs[u] * 64 + lane;
                    }
                    count += __popcll(m);
                }
            }
        }
        if (lane == 0) rec[g] = kept;
    }
    if (lane == 0) counts[r] = count;
    if (HEAD) {
        const int have = count < ho.K ? count : ho.K;
        if (lane == 0) { ho.packed[2 * r] = (int32_t)(r * ho.K); ho.packed[2 * r + 1] = have; }
        __builtin_amdgcn_wave_barrier();
        if (lane < have) {                                       // the head rows: ONE copy of this code, outside the (unrolled) chunk loop
            const int64_t pos = r * ho.K + lane;
            const int k = s_head[wv][lane];
            const float a = lat(k), b = mp.lattice_mode == PERF_LATTICE_REPEATED ? add_rn(a, mp.step) : lattice_single(t0, k + 1, mp.step);
            ho.ts[pos] = a; ho.te[pos] = b; ho.ri[pos] = r;
            sample_point_store(ro + 3 * r, rd + 3 * r, a, b, ho.bb, ho.x01, ho.sel, pos);
        }
        if (lane >= have && lane < ho.K) {                       // padding rows: harmless inputs, selector 0
            const int64_t pos = r * ho.K + lane;
            ho.ts[pos] = 0.f; ho.te[pos] = 0.f; ho.ri[pos] = r;
            ho.x01[3 * pos] = 0.5f; ho.x01[3 * pos + 1] = 0.5f; ho.x01[3 * pos + 2] = 0.5f; ho.sel[pos] = 0;
        }
    }
}

// The write pass of workgroup `block` of `n_blocks` (256 threads) -- march_write_kernel is this body.
__device__ __forceinline__ void march_write_body(int block, int n_blocks, const float* __restrict__ t0s, int64_t n_rays, float step,
                                                 int32_t mask_words, const uint64_t* __restrict__ masks,
                                                 const int32_t* __restrict__ counts,
                                                 const int32_t* __restrict__ offsets, int64_t capacity,
                                                 int64_t* __restrict__ ray_indices, float* __restrict__ ts,
                                                 float* __restrict__ te, int32_t* __restrict__ packed,
                                                 const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                 const Aabb& bb, float* __restrict__ x01, uint8_t* __restrict__ sel,
                                                 int32_t rank_lo, float t0_scale, float t0_base, int lattice_mode, const SharedRuns& sr,
                                                 const float* __restrict__ lat_full) {
    // (all rays on one lattice -- eval renders --: the host-built table of runs, see march_count_kernel; per-ray origins walk)
    __shared__ int32_t w_ks[kMaxRuns];
    __shared__ uint32_t w_bs[kMaxRuns], w_dd[kMaxRuns];
    if (sr.n > 0) {
        if ((int)threadIdx.x < sr.n) { w_ks[threadIdx.x] = sr.ks[threadIdx.x]; w_bs[threadIdx.x] = sr.bs[threadIdx.x]; w_dd[threadIdx.x] = sr.dd[threadIdx.x]; }
        __syncthreads();
    }
    const int32_t* ray_rows = (t0s && lat_full) ? reinterpret_cast<const int32_t*>(lat_full) : nullptr;      // per-ray tables (see march_count_kernel)
    if (ray_rows) lat_full = nullptr;
    LatticeRuns tab;
    tab.n = sr.n; tab.ks = w_ks; tab.bs = w_bs; tab.dd = w_dd; tab.t0 = 0.f; tab.step = step; tab.mode = lattice_mode; tab.full = lat_full;
    // Writes the samples of rank [rank_lo, rank_lo + counts[r]) of every ray (rank = position among the ray's samples in t
    // order) to offsets[r]...: rank_lo = 0 and counts = the march counts is the plain expansion; the two-phase sampler
    // writes the first K samples of every ray first and the rest of the rays that are still alive later.
    // With at most 16 samples to write for each ray of an aligned group of four, every ray gets a quarter wave whose lanes
    // walk the 64 bits of a mask word in four steps; otherwise every ray has its own wave (the kernel has no cross-lane
    // operation: a team is only a lane -> (ray, bit) mapping).
    // (two launch shapes as in composite.hip:for_rays_of_wave: n_rays / 4 waves for large batches -- wave w serves rays
    //  4w..4w+3 --, one wave per ray for small ones, where in the quarter-wave case the first wave of an aligned group of
    //  four rays serves all four and the other three retire at once)
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)block * 4 + (threadIdx.x >> 6);
    const bool four_per_wave = (int64_t)n_blocks * 4 < n_rays;          // n_rays / 4 waves launched (large batches), else one per ray
    const int64_t r0 = four_per_wave ? w * 4 : (w & ~(int64_t)3);
    if (r0 >= n_rays) return;
    const int64_t rq = r0 + (lane >> 4);
    const bool small = __ballot(rq < n_rays && counts[rq] > 16) == 0ull;
    if (small && !four_per_wave && (w & 3) != 0) return;
    const int W = small ? 16 : 64;
    const int l = small ? (lane & 15) : lane;
    for (int q = 0; q < ((four_per_wave && !small) ? 4 : 1); ++q) {
        const int64_t r = small ? rq : (four_per_wave ? r0 + q : w);
        if (r >= n_rays) continue;
        int32_t cnt = counts[r];
        const int32_t off = offsets[r];
        if ((int64_t)off + cnt > capacity) cnt = (int32_t)(capacity > off ? capacity - off : 0);   // truncated batch
        if (l == 0) { packed[2 * r] = off; packed[2 * r + 1] = cnt; }
        if (cnt == 0) continue;
        const float t0 = lattice_origin(t0s, r, t0_scale, t0_base);
        int64_t run = (int64_t)off - rank_lo;            // output position of rank 0 (may lie before `off`)
        const int64_t end = (int64_t)off + cnt;
        const int nlw = n_live_words(mask_words);
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
                        const float a = lat_full ? lat_full[k]
                                                 : (tab.n > 0 ? tab.at(tab.find(k), k)
                                                              : ((ray_rows && lattice_mode == PERF_LATTICE_REPEATED) ? runs_row_at(ray_rows + r * (int64_t)kRunsStride, k, t0, step)
                                                                                                                     : lattice(t0, k, step, lattice_mode)));
                        const float b = lattice_mode == PERF_LATTICE_REPEATED ? add_rn(a, step) : lattice_single(t0, k + 1, step);
                        ts[pos] = a;
                        te[pos] = b;
                        ray_indices[pos] = r;
                        if (x01) sample_point_store(rays_o + 3 * r, rays_d + 3 * r, a, b, bb, x01, sel, pos);     // (= perf_points_from_rays)
                    }
                }
                run += __popcll(m);
            }
        }
    }
}

// One LANE per ray.  The walk as a loop WITHOUT long divergent bodies: every iteration makes the two real additions and the
// division whatever happens next (lanes cross their binades at different indices; with the three cases as branches a wave
// executed all three bodies in nearly every iteration: 31 us for 8,192 rays), then advances by one of the three cases.  Same
// arithmetic, same tables as lattice_runs_build.
__device__ __forceinline__ int lattice_runs_build_lane(float t0, float step, int k_need, int32_t* __restrict__ row) {
    int32_t* ks = row + 1;
    uint32_t* bs = reinterpret_cast<uint32_t*>(row + 1 + kMaxRuns);
    uint32_t* dd = reinterpret_cast<uint32_t*>(row + 1 + 2 * kMaxRuns);
    int n = 0;
    uint32_t tb = __float_as_uint(t0);
    ks[0] = 0; bs[0] = tb; dd[0] = 0u; n = 1;
    int K = 0;
    bool stuck = false;
    while (K < k_need && !stuck) {
        if (n + 2 > kMaxRuns) return -1;
        const uint32_t b1 = __float_as_uint(add_rn(__uint_as_float(tb), step));
        const uint32_t b2 = __float_as_uint(add_rn(__uint_as_float(b1), step));
        const bool c1 = (b1 >> 23) != (tb >> 23);            // the first addition entered a binade: one more real step first
        const bool c2 = (b2 >> 23) != (b1 >> 23);
        const uint32_t d = b2 - b1;
        const uint32_t top = (b2 & 0xff800000u) + 0x00800000u;
        const uint32_t j = div_u24(top - 1u - b2, d ? d : 1u);
        // run K+1 (always emitted): a single point (c1, c2) or the arithmetic run to the end of the binade
        ks[n] = K + 1; bs[n] = b1; dd[n] = (c1 || c2) ? 0u : d;
        ++n;
        if (!c1 && c2) { ks[n] = K + 2; bs[n] = b2; dd[n] = 0u; ++n; }
        stuck = !c1 && !c2 && d == 0u;                       // (step below half an ulp: the lattice stays at t_{K+1} for good)
        tb = c1 ? b1 : (c2 ? b2 : b2 + j * d);
        K += c1 ? 1 : (c2 ? 2 : 2 + (int)j);
    }
    return n;
}

// row r of the per-ray tables (one LANE per ray) -- lattice_runs_kernel is this body
__device__ __forceinline__ void lattice_runs_row(int64_t r, const float* __restrict__ t0s, float t0_scale, float t0_base, int64_t n_rays,
                                                 float step, int32_t k_need, int32_t* __restrict__ rows) {
    if (r >= n_rays) return;
    int32_t* row = rows + r * (int64_t)kRunsStride;
    row[0] = lattice_runs_build_lane(lattice_origin(t0s, r, t0_scale, t0_base), step, k_need, row);
}

}  // namespace perf
