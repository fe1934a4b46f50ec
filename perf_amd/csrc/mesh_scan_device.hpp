// What the mesh units (mesh.hip, brickmesh.hip, meshcc.hip, meshvis.hip, meshsimp.hip) compact their streams with: the exclusive scan
// of uint64 words in levels of 256 and the rank of a flagged thread inside its workgroup of 256 (the host checks are mesh_check_host.hpp's).
// The kernels have internal linkage: every unit that includes this header registers its own copies with the runtime.
#pragma once
#include "common.hpp"
#include "mesh_check_host.hpp"

namespace perf {

constexpr int kScanGroup = 256;              // items of one workgroup: one per thread; the scan's fan-in

// words of the scan's levels above n items: n1 = ceil(n / 256), n2 = ceil(n1 / 256), ... down to a level of one word (the total)
static inline int64_t scan_words(int64_t n) {
    int64_t words = 0;
    do {
        n = div_up(n, kScanGroup);
        words += n;
    } while (n > 1);
    return words;
}

// S(n) of the headers: the counts of the groups of 256 of n items and the levels of their scan
static inline int64_t group_words(int64_t n) {
    if (n == 0) return 0;
    const int64_t groups = div_up(n, kScanGroup);
    return groups + scan_words(groups);
}

static inline unsigned scan_groups(int64_t n) { return (unsigned)div_up(n, kScanGroup); }

struct ScanNoTail {
    __device__ void operator()(uint64_t) const {}
};

namespace {

// One level of the scan: the exclusive prefix of each run of 256 words in place, the run's sum to sums[block].  top (the level of one
// workgroup): thread 0 hands the grand total to tail.
template <class Tail>
__global__ void __launch_bounds__(kScanGroup) scan_kernel(uint64_t* __restrict__ data, int64_t n, uint64_t* __restrict__ sums, Tail tail, bool top) {
    __shared__ uint64_t wave_sum[kScanGroup / 64];
    const int64_t idx = (int64_t)blockIdx.x * kScanGroup + threadIdx.x;
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t own = idx < n ? data[idx] : 0;
    uint64_t incl = own;
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (int w = 0; w < kScanGroup / 64; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    if (idx < n) data[idx] = before + incl - own;
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        if (top) tail(total);
    }
}

__global__ void __launch_bounds__(kScanGroup) scan_add_kernel(uint64_t* __restrict__ data, int64_t n, const uint64_t* __restrict__ prefix) {
    const int64_t idx = (int64_t)blockIdx.x * kScanGroup + threadIdx.x;
    if (idx < n) data[idx] += prefix[blockIdx.x];
}

}  // namespace

// Scans data [n] in place (n >= 1) with its levels in `level` (scan_words(n) words) -> the word that holds the grand total.  Up the
// levels: each level's runs of 256 are scanned in place and their sums become the next level; the level of one word is the total, which
// the launch that writes it also hands to tail.  And down again: a level's run takes the prefix of its sum (the level under the top has
// one run, whose prefix is zero).
template <class Tail = ScanNoTail>
static const uint64_t* scan_u64(uint64_t* data, int64_t n, uint64_t* level, hipStream_t st, Tail tail = {}) {
    uint64_t* at[8]; int64_t count[8];
    int levels = 0;
    at[0] = data; count[0] = n;
    while (true) {
        const int64_t blocks = div_up(count[levels], kScanGroup);
        hipLaunchKernelGGL(scan_kernel<Tail>, dim3((unsigned)blocks), dim3(kScanGroup), 0, st, at[levels], count[levels], level, tail, blocks == 1);
        at[levels + 1] = level; count[levels + 1] = blocks;
        level += blocks;
        ++levels;
        if (blocks == 1) break;
    }
    for (int l = levels - 2; l >= 0; --l)
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)count[l + 1]), dim3(kScanGroup), 0, st, at[l], count[l], at[l + 1]);
    return at[levels];
}

// The rank of a flagged thread among the flagged threads of its workgroup of 256, and the workgroup's count to sums[blockIdx.x].
// All 256 threads arrive.
__device__ __forceinline__ int32_t group_rank(bool flag, uint64_t* __restrict__ sums) {
    __shared__ int32_t wave_sum[kScanGroup / 64];
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t mask = __ballot(flag);
    if (lane == 0) wave_sum[wave] = __popcll(mask);
    __syncthreads();
    int32_t before = 0, total = 0;
    for (int w = 0; w < kScanGroup / 64; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    if (sums && threadIdx.x == 0) sums[blockIdx.x] = (uint64_t)total;
    return before + __popcll(mask & ((1ull << lane) - 1));
}

}  // namespace perf
