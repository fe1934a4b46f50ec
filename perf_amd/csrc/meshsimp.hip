// Vertex clustering of a triangle mesh (include/perf_hip_meshsimp.h): bounds; keys -> insert -> smallest -> scan -> ids; sums -> mean ->
// nearest -> representative -> finish; remap -> insert -> resolve.  The two inserts are wait-free hash sets: a slot goes EMPTY -> member
// by one compare-and-swap and only falls afterwards, by atomicMin of members of the same key; a failed compare-and-swap goes on from the
// value it returned; the occupant's key is read from an array an earlier launch wrote (the header has the argument).
#include "common.hpp"
#include "mesh_scan_device.hpp"
#include "../../include/perf_hip_meshsimp.h"

namespace perf {

constexpr int kSgGroup = kScanGroup;         // items of one workgroup: one per thread (group_rank's workgroup)
constexpr int kSgPlaceGroup = 1024;          // sums, nearest: a workgroup of 16 waves joins its waves' runs before the atomics
constexpr int kSgBoundsPerThread = 8;        // bounds: vertices one thread takes before the wave's six atomics
constexpr uint32_t kSgEmpty = 0xffffffffu;
constexpr uint64_t kSgMul = 0x9E3779B97F4A7C15ull;

struct SgGrid {
    double lo[3];
    double h;
    int32_t n[3];
};

// T(n) of the header, as its log2
static inline int sg_table_bits(int64_t n) {
    int bits = 8;
    while (((int64_t)1 << bits) < 2 * n) ++bits;
    return bits;
}

struct SgLayout {
    int64_t* keys;           // [V] the vertices' keys, -1 for a vertex that joins nothing
    uint64_t* vsums;         // S(V)
    int64_t* totals;         // [4] (C, first bad vertex, -, -)
    uint32_t* slot;          // [V] the slot of each vertex's key, then the ranks within their groups of the clusters' smallest members
    int32_t* smallest;       // [V] the smallest member of each vertex's cluster
    uint32_t* vtable;        // [T(V)]
    uint32_t* fslot;         // [F'] the slot of each kept face's canonical triple
    uint32_t* ftable;        // [T(F)]
    int64_t bytes;
};

static inline SgLayout sg_layout(void* workspace, int64_t n_vertices, int64_t n_faces) {
    SgLayout l;
    const uintptr_t base = reinterpret_cast<uintptr_t>(workspace);
    int64_t at = 0;
    l.keys = reinterpret_cast<int64_t*>(base + at);       at += 8 * n_vertices;
    l.vsums = reinterpret_cast<uint64_t*>(base + at);     at += 8 * group_words(n_vertices);
    l.totals = reinterpret_cast<int64_t*>(base + at);     at += 8 * 4;
    l.slot = reinterpret_cast<uint32_t*>(base + at);      at += 4 * n_vertices;
    l.smallest = reinterpret_cast<int32_t*>(base + at);   at += 4 * n_vertices;
    l.vtable = reinterpret_cast<uint32_t*>(base + at);    at += 4 * ((int64_t)1 << sg_table_bits(n_vertices));
    l.fslot = reinterpret_cast<uint32_t*>(base + at);     at += 4 * ((n_faces + 1) & ~(int64_t)1);
    l.ftable = reinterpret_cast<uint32_t*>(base + at);    at += 4 * ((int64_t)1 << sg_table_bits(n_faces));
    l.bytes = (at + 15) & ~(int64_t)15;
    return l;
}

// ---- runs of one id along a wave ------------------------------------------------------------------------------------------------------------
// The lane that starts the run of equal ids this lane is in (ids of neighbouring lanes are compared; every lane of the wave arrives).
__device__ __forceinline__ int sg_run_head(int64_t id, int lane) {
    const int64_t before = __shfl_up((long long)id, 1);
    const uint64_t heads = __ballot(lane == 0 || before != id);          // (bit 0 is always set)
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
    return 63 - __clzll((long long)(heads & upto));
}

// whether the next lane starts another run
__device__ __forceinline__ bool sg_run_tail(int64_t id, int lane) {
    const int64_t after = __shfl_down((long long)id, 1);
    return lane == 63 || after != id;
}

// Joins the runs of the waves of a workgroup of kSgPlaceGroup threads: val [N] is what a run's lanes hold after the wave's segmented scan
// (its last lane: the run's sums, or minima with kMin).  The last run of a wave is CARRIED into the next wave when that one starts with
// the same id, and on through every wave that is one run of that id: where all the vertices of a workgroup share a cell, one lane of the
// 1,024 goes to memory.  -> whether this lane is the one that takes its run's val, now with what was carried into it, to memory.
// Integers and minima: exact in any grouping.  All threads arrive.
template <int N, bool kMin>
__device__ __forceinline__ bool sg_join_waves(int32_t c, int lane, int head, bool tail, unsigned long long val[N]) {
    constexpr int kWaves = kSgPlaceGroup / 64;
    __shared__ int32_t first_id[kWaves], last_id[kWaves], whole[kWaves];
    __shared__ unsigned long long last_val[kWaves][N];
    const int wave = threadIdx.x >> 6;
    if (lane == 0) first_id[wave] = c;
    if (lane == 63) {
        last_id[wave] = c;
        whole[wave] = head == 0;
        for (int k = 0; k < N; ++k) last_val[wave][k] = val[k];
    }
    __syncthreads();
    if (!tail || c < 0) return false;
    if (lane == 63 && wave + 1 < kWaves && first_id[wave + 1] == c) return false;          // carried into the next wave
    if (head == 0)                                          // the wave's first run: what the waves before it carried
        for (int u = wave - 1; u >= 0 && last_id[u] == c; --u) {
            for (int k = 0; k < N; ++k) val[k] = kMin ? (last_val[u][k] < val[k] ? last_val[u][k] : val[k]) : val[k] + last_val[u][k];
            if (!whole[u]) break;
        }
    return true;
}

// ---- the cell rule --------------------------------------------------------------------------------------------------------------------------
// -> false for a vertex with a coordinate that is not finite.  cell [3]: the cell's indices, q [3]: the fixed-point fractions.
__device__ __forceinline__ bool sg_cell(const float* __restrict__ vertices, int64_t v, const SgGrid& g, int64_t cell[3], int64_t q[3]) {
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        const float x = vertices[3 * v + a];
        if (!__builtin_isfinite(x)) { finite = false; cell[a] = 0; q[a] = 0; continue; }
        const double n = (double)g.n[a];
        double t = ((double)x - g.lo[a]) / g.h;
        t = t > 0.0 ? t : 0.0;
        t = t < n ? t : n;
        int64_t i = (int64_t)floor(t);
        if (i > g.n[a] - 1) i = g.n[a] - 1;
        const double f = t - (double)i;
        cell[a] = i;
        q[a] = (int64_t)llrint(f * 4294967296.0);
    }
    return finite;
}

__device__ __forceinline__ uint64_t sg_cell_hash(int64_t key, int bits) { return ((uint64_t)key * kSgMul) >> (64 - bits); }

// One member into a set (the header has the argument).  same(j): whether member j, read from the table, has this member's key.
// -> the slot of the key.  The walk passes only slots of other keys, fewer than there are slots; the bound is the table's size.
template <class SameKey>
__device__ __forceinline__ uint64_t sg_insert(uint32_t* table, uint64_t mask, uint64_t slot, uint32_t member, SameKey same) {
    for (uint64_t step = 0; step <= mask; ++step) {
        uint32_t seen = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == kSgEmpty) {
            seen = atomicCAS(table + slot, kSgEmpty, member);
            if (seen == kSgEmpty) return slot;              // the slot is this key's now
        }
        if (same(seen)) {                                   // seen: a member, as loaded or as the compare-and-swap returned it
            atomicMin(table + slot, member);
            return slot;
        }
        slot = (slot + 1) & mask;
    }
    return slot;
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------------------------
// an order-preserving image of the finite floats in the signed integers
__device__ __forceinline__ int32_t sg_ordered(float x) {
    const int32_t b = __float_as_int(x);
    return b >= 0 ? b : b ^ 0x7fffffff;
}

__global__ void meshsimp_bounds_init_kernel(int32_t* __restrict__ image) {
    if (threadIdx.x < 6 && blockIdx.x == 0) image[threadIdx.x] = threadIdx.x < 3 ? 0x7fffffff : (int32_t)0x80000000;
}

__global__ void __launch_bounds__(kSgGroup) meshsimp_bounds_kernel(const float* __restrict__ vertices, int64_t n_vertices, int32_t* __restrict__ image) {
    const int64_t base = (int64_t)blockIdx.x * (kSgGroup * kSgBoundsPerThread) + threadIdx.x;
    int32_t low[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, high[3] = {(int32_t)0x80000000, (int32_t)0x80000000, (int32_t)0x80000000};
    for (int k = 0; k < kSgBoundsPerThread; ++k) {
        const int64_t v = base + (int64_t)k * kSgGroup;
        if (v >= n_vertices) break;
        for (int a = 0; a < 3; ++a) {
            const float x = vertices[3 * v + a];
            if (!__builtin_isfinite(x)) continue;
            const int32_t o = sg_ordered(x);
            low[a] = o < low[a] ? o : low[a];
            high[a] = o > high[a] ? o : high[a];
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) {
            const int32_t l = __shfl_xor(low[a], off), h = __shfl_xor(high[a], off);
            low[a] = l < low[a] ? l : low[a];
            high[a] = h > high[a] ? h : high[a];
        }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) {
            if (low[a] != 0x7fffffff) atomicMin(image + a, low[a]);
            if (high[a] != (int32_t)0x80000000) atomicMax(image + 3 + a, high[a]);
        }
}

// the images back to floats, in place
__global__ void meshsimp_bounds_finish_kernel(int32_t* __restrict__ image) {
    if (threadIdx.x >= 3 || blockIdx.x != 0) return;
    const int32_t l = image[threadIdx.x], h = image[3 + threadIdx.x];
    const bool none = l > h;
    image[threadIdx.x] = none ? 0x7f800000 : (l >= 0 ? l : l ^ 0x7fffffff);
    image[3 + threadIdx.x] = none ? (int32_t)0xff800000 : (h >= 0 ? h : h ^ 0x7fffffff);
}

// ---- cluster --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSgGroup) meshsimp_keys_kernel(const float* __restrict__ vertices, int64_t n_vertices, SgGrid grid, int64_t* __restrict__ keys,
                                                                 unsigned long long* __restrict__ first_bad) {
    const int64_t v = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (v >= n_vertices) return;
    int64_t cell[3], q[3];
    if (sg_cell(vertices, v, grid, cell, q)) {
        keys[v] = cell[0] << 42 | cell[1] << 21 | cell[2];
    } else {
        keys[v] = -1;
        atomicMin(first_bad, (unsigned long long)v);
    }
}

// Of the vertices of a wave that follow one another with one key, the first goes to the table (it is the smallest of them) and hands the
// slot to the others.
__global__ void __launch_bounds__(kSgGroup) meshsimp_insert_cells_kernel(const int64_t* __restrict__ keys, int64_t n_vertices, uint32_t* table, int bits,
                                                                         uint32_t* __restrict__ slot_of) {
    const int64_t v = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t key = v < n_vertices ? keys[v] : -1;
    const int head = sg_run_head(key, lane);
    uint32_t slot = 0;
    if (head == lane && key >= 0)
        slot = (uint32_t)sg_insert(table, ((uint64_t)1 << bits) - 1, sg_cell_hash(key, bits), (uint32_t)v,
                                   [&](uint32_t j) { return (int64_t)j < n_vertices && keys[j] == key; });
    slot = __shfl(slot, head);
    if (key >= 0) slot_of[v] = slot;
}

// smallest[v] = the smallest member of v's cluster (what the insert's launch left in the key's slot); rank[v] (over slot_of, which is read
// first) = the rank of v among the smallest members of its group; the group's count to sums
__global__ void __launch_bounds__(kSgGroup) meshsimp_smallest_kernel(const int64_t* __restrict__ keys, const uint32_t* __restrict__ table, int64_t n_vertices,
                                                                     uint32_t* __restrict__ slot_then_rank, int32_t* __restrict__ smallest,
                                                                     uint64_t* __restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    int64_t s = -1;
    if (v < n_vertices && keys[v] >= 0) {
        s = table[slot_then_rank[v]];
        if (s > v) s = v;                                   // (s is in [0, v]: v itself took part in the minimum)
    }
    const int32_t r = group_rank(s == v && v < n_vertices, sums);
    if (v < n_vertices) {
        smallest[v] = (int32_t)s;
        slot_then_rank[v] = (uint32_t)r;
    }
}

__global__ void __launch_bounds__(kSgGroup) meshsimp_ids_kernel(const int32_t* __restrict__ smallest, const uint32_t* __restrict__ rank,
                                                                const uint64_t* __restrict__ prefix, int64_t n_vertices, int32_t* __restrict__ vertex_cluster) {
    const int64_t v = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (v >= n_vertices) return;
    const int32_t s = smallest[v];                          // -1, or in [0, v]
    vertex_cluster[v] = s < 0 ? -1 : (int32_t)prefix[s / kSgGroup] + (int32_t)rank[s];
}

__global__ void meshsimp_totals_kernel(const uint64_t* __restrict__ total, int64_t* __restrict__ totals, int64_t* __restrict__ counts_dev) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t c = total ? (int64_t)total[0] : 0;
    totals[0] = c;
    counts_dev[0] = c; counts_dev[1] = totals[1];
}

// ---- place ----------------------------------------------------------------------------------------------------------------------------------
struct SgScratch {
    unsigned long long* sums;    // [3 C] the sums of q; then, as doubles, p
    unsigned long long* count;   // [C]
    int64_t* key;                // [C]
    unsigned long long* best;    // [C] the bits of the smallest d2 (d2 >= 0: the bits order as the values)
};

static inline SgScratch sg_scratch(void* scratch, int64_t n_clusters) {
    SgScratch s;
    s.sums = (unsigned long long*)scratch;
    s.count = s.sums + 3 * n_clusters;
    s.key = (int64_t*)(s.count + n_clusters);
    s.best = (unsigned long long*)(s.key + n_clusters);
    return s;
}

// The sums of a run of vertices of one cluster are formed inside the wave, the waves' runs joined across the workgroup (integers: exact in
// any order); the run's last lane adds them.
__global__ void __launch_bounds__(kSgPlaceGroup) meshsimp_sums_kernel(const float* __restrict__ vertices, int64_t n_vertices, SgGrid grid,
                                                                      const int32_t* __restrict__ vertex_cluster, int64_t n_clusters, SgScratch out) {
    const int64_t v = (int64_t)blockIdx.x * kSgPlaceGroup + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int64_t cell[3] = {0, 0, 0}, q[3] = {0, 0, 0};
    int32_t c = -1;
    if (v < n_vertices) {
        c = vertex_cluster[v];
        if (c < 0 || c >= n_clusters || !sg_cell(vertices, v, grid, cell, q)) c = -1;
    }
    const int head = sg_run_head(c, lane);
    for (int off = 1; off < 64; off <<= 1)
        for (int a = 0; a < 3; ++a) {
            const int64_t up = __shfl_up((long long)q[a], off);
            if (lane - off >= head) q[a] += up;
        }
    unsigned long long val[4] = {(unsigned long long)q[0], (unsigned long long)q[1], (unsigned long long)q[2], (unsigned long long)(lane - head + 1)};
    if (!sg_join_waves<4, false>(c, lane, head, sg_run_tail(c, lane), val)) return;
    for (int a = 0; a < 3; ++a) atomicAdd(out.sums + 3 * (int64_t)c + a, val[a]);
    atomicAdd(out.count + c, val[3]);
    out.key[c] = cell[0] << 42 | cell[1] << 21 | cell[2];          // (every member stores the same value)
}

__global__ void __launch_bounds__(kSgGroup) meshsimp_mean_kernel(SgGrid grid, int64_t n_clusters, SgScratch s, int32_t placement, float* __restrict__ cluster_vertices,
                                                                 int32_t* __restrict__ representative) {
    const int64_t c = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (c >= n_clusters) return;
    const double count = (double)s.count[c];
    const int64_t key = s.key[c];
    const int64_t cell[3] = {key >> 42, (key >> 21) & 0x1fffff, key & 0x1fffff};
    double* p = (double*)s.sums;
    for (int a = 0; a < 3; ++a) {
        const double sum = (double)(int64_t)s.sums[3 * c + a];
        const double m = count > 0.0 ? sum / (count * 4294967296.0) : 0.0;
        const double at = grid.lo[a] + ((double)cell[a] + m) * grid.h;
        p[3 * c + a] = at;
        if (placement == PERF_MESHSIMP_PLACE_MEAN) cluster_vertices[3 * c + a] = (float)at;
    }
    representative[c] = 0x7fffffff;
}

__device__ __forceinline__ unsigned long long sg_distance_bits(const float* __restrict__ vertices, int64_t v, const double* __restrict__ p, int64_t c) {
    const double dx = (double)vertices[3 * v] - p[3 * c], dy = (double)vertices[3 * v + 1] - p[3 * c + 1], dz = (double)vertices[3 * v + 2] - p[3 * c + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return (unsigned long long)__double_as_longlong(d2);
}

__device__ __forceinline__ int32_t sg_member_of(const float* __restrict__ vertices, int64_t v, int64_t n_vertices, const int32_t* __restrict__ vertex_cluster,
                                                int64_t n_clusters) {
    if (v >= n_vertices) return -1;
    const int32_t c = vertex_cluster[v];
    if (c < 0 || c >= n_clusters) return -1;
    return __builtin_isfinite(vertices[3 * v]) && __builtin_isfinite(vertices[3 * v + 1]) && __builtin_isfinite(vertices[3 * v + 2]) ? c : -1;
}

// the smallest d2 of a run of vertices of one cluster inside the wave, the waves' runs joined across the workgroup; the run's last lane
// takes it to the cluster's word
__global__ void __launch_bounds__(kSgPlaceGroup) meshsimp_nearest_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                         const int32_t* __restrict__ vertex_cluster, int64_t n_clusters, SgScratch s) {
    const int64_t v = (int64_t)blockIdx.x * kSgPlaceGroup + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t c = sg_member_of(vertices, v, n_vertices, vertex_cluster, n_clusters);
    unsigned long long bits[1] = {c >= 0 ? sg_distance_bits(vertices, v, (const double*)s.sums, c) : ~0ull};
    const int head = sg_run_head(c, lane);
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(bits[0], off);
        if (lane - off >= head && up < bits[0]) bits[0] = up;
    }
    if (sg_join_waves<1, true>(c, lane, head, sg_run_tail(c, lane), bits)) atomicMin(s.best + c, bits[0]);
}

// the members at the smallest d2 (one, but for ties) take the minimum of their indices
__global__ void __launch_bounds__(kSgGroup) meshsimp_representative_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                           const int32_t* __restrict__ vertex_cluster, int64_t n_clusters, SgScratch s,
                                                                           int32_t* __restrict__ representative) {
    const int64_t v = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    const int32_t c = sg_member_of(vertices, v, n_vertices, vertex_cluster, n_clusters);
    if (c < 0) return;
    if (sg_distance_bits(vertices, v, (const double*)s.sums, c) == s.best[c]) atomicMin(representative + c, (int32_t)v);
}

__global__ void __launch_bounds__(kSgGroup) meshsimp_finish_kernel(const float* __restrict__ vertices, int64_t n_vertices, int64_t n_clusters, int32_t placement,
                                                                   float* __restrict__ cluster_vertices, int32_t* __restrict__ representative) {
    const int64_t c = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (c >= n_clusters) return;
    const int32_t r = representative[c];
    if (r < 0 || r >= n_vertices) {                         // an id without members
        representative[c] = -1;
        return;
    }
    if (placement != PERF_MESHSIMP_PLACE_MEMBER) return;
    for (int a = 0; a < 3; ++a) cluster_vertices[3 * c + a] = vertices[3 * (int64_t)r + a];
}

// ---- faces ----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSgGroup) meshsimp_remap_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ vertex_cluster,
                                                                  int64_t n_vertices, int32_t* __restrict__ faces_out, uint8_t* __restrict__ face_keep,
                                                                  unsigned long long* __restrict__ first_bad) {
    const int64_t f = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int32_t ca = -1, cb = -1, cc = -1;
    if (a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices) {
        ca = vertex_cluster[a]; cb = vertex_cluster[b]; cc = vertex_cluster[c];
    } else {
        atomicMin(first_bad, (unsigned long long)f);
    }
    faces_out[3 * f] = ca; faces_out[3 * f + 1] = cb; faces_out[3 * f + 2] = cc;
    face_keep[f] = ca >= 0 && cb >= 0 && cc >= 0 && ca != cb && cb != cc && ca != cc;
}

struct SgTriple {
    int32_t a, b, c;
};

// the canonical triple of a remapped face with three different ids
template <bool kSorted>
__device__ __forceinline__ SgTriple sg_canonical(const int32_t* __restrict__ remapped, int64_t f) {
    int32_t a = remapped[3 * f], b = remapped[3 * f + 1], c = remapped[3 * f + 2];
    if (b < a && b < c) { const int32_t t = a; a = b; b = c; c = t; }                  // rotate the smallest id to the front
    else if (c < a && c < b) { const int32_t t = c; c = b; b = a; a = t; }
    if (kSorted && c < b) { const int32_t t = b; b = c; c = t; }
    return {a, b, c};
}

template <bool kSorted>
__global__ void __launch_bounds__(kSgGroup) meshsimp_insert_faces_kernel(const int32_t* __restrict__ remapped, const uint8_t* __restrict__ face_keep, int64_t n_faces,
                                                                         uint32_t* table, int bits, uint32_t* __restrict__ slot_of) {
    const int64_t f = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (f >= n_faces || !face_keep[f]) return;
    const SgTriple mine = sg_canonical<kSorted>(remapped, f);
    const uint64_t mask = ((uint64_t)1 << bits) - 1;
    const uint64_t start = (((((uint64_t)(uint32_t)mine.a << 32 | (uint32_t)mine.b) * kSgMul) >> (64 - bits)) + (uint64_t)(uint32_t)mine.c) & mask;
    slot_of[f] = (uint32_t)sg_insert(table, mask, start, (uint32_t)f, [&](uint32_t j) {
        if ((int64_t)j >= n_faces) return false;
        const SgTriple other = sg_canonical<kSorted>(remapped, j);
        return other.a == mine.a && other.b == mine.b && other.c == mine.c;
    });
}

__global__ void __launch_bounds__(kSgGroup) meshsimp_resolve_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ slot_of, int64_t n_faces,
                                                                    uint8_t* __restrict__ face_keep) {
    const int64_t f = (int64_t)blockIdx.x * kSgGroup + threadIdx.x;
    if (f >= n_faces || !face_keep[f]) return;
    face_keep[f] = table[slot_of[f]] == (uint32_t)f;
}

// ---- the checks of the entry points -----------------------------------------------------------------------------------------------------------
static int sg_counts_check(const char* who, int64_t n_vertices, int64_t n_faces) {
    return mesh_counts_check(who, n_vertices, n_faces, PERF_MESHSIMP_MAX_VERTICES, PERF_MESHSIMP_MAX_FACES, "2^31 - 1 (the face set holds int32 face indices)");
}

static int sg_grid_check(const char* who, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz, SgGrid* grid) {
    PERF_REQUIRE(lo, "%s: NULL input (lo)", who);
    PERF_REQUIRE(std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2]), "%s: the grid's origin lo is not finite", who);
    PERF_REQUIRE(std::isfinite(h) && h > 0.0f, "%s: the cell edge h (%g) is not positive or not finite", who, (double)h);
    const int32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        PERF_REQUIRE(n[a] >= 1 && n[a] <= PERF_MESHSIMP_MAX_CELLS, "%s: %d cells along axis %d are outside 1 .. 2^21", who, (int)n[a], a);
        grid->lo[a] = (double)lo[a];
        grid->n[a] = n[a];
    }
    grid->h = (double)h;
    return PERF_OK;
}

static int sg_workspace_check(const char* who, int64_t n_vertices, int64_t n_faces, const void* workspace, int64_t workspace_bytes) {
    return workspace_check(who, perf_meshsimp_workspace_bytes(n_vertices, n_faces), workspace, workspace_bytes);
}

}  // namespace perf

using namespace perf;

extern "C" int perf_meshsimp_version(void) { return PERF_MESHSIMP_ABI_VERSION; }

extern "C" int64_t perf_meshsimp_table_slots(int64_t n) {
    if (n < 0 || n > PERF_MESHSIMP_MAX_FACES) {
        set_error("perf_meshsimp_table_slots: %lld members are outside 0 .. 2^31 - 1", (long long)n);
        return -1;
    }
    return (int64_t)1 << sg_table_bits(n);
}

extern "C" int64_t perf_meshsimp_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (sg_counts_check("perf_meshsimp_workspace_bytes", n_vertices, n_faces) != PERF_OK) return -1;
    return sg_layout(nullptr, n_vertices, n_faces).bytes;
}

extern "C" int perf_meshsimp_bounds(const float* vertices, int64_t n_vertices, float* bounds_dev, void* stream) {
    if (int rc = sg_counts_check("perf_meshsimp_bounds", n_vertices, 0)) return rc;
    PERF_REQUIRE(vertices || n_vertices == 0, "perf_meshsimp_bounds: NULL input (vertices) with vertices to bound");
    PERF_REQUIRE(bounds_dev, "perf_meshsimp_bounds: NULL output (bounds_dev)");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(meshsimp_bounds_init_kernel, dim3(1), dim3(64), 0, st, (int32_t*)bounds_dev);
    if (n_vertices > 0)
        hipLaunchKernelGGL(meshsimp_bounds_kernel, dim3((unsigned)div_up(n_vertices, kSgGroup * kSgBoundsPerThread)), dim3(kSgGroup), 0, st, vertices, n_vertices,
                           (int32_t*)bounds_dev);
    hipLaunchKernelGGL(meshsimp_bounds_finish_kernel, dim3(1), dim3(64), 0, st, (int32_t*)bounds_dev);
    PERF_LAUNCH_CHECK("perf_meshsimp_bounds");
    return PERF_OK;
}

extern "C" int perf_meshsimp_cluster(const float* vertices, int64_t n_vertices, int64_t n_faces, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz,
                                     int32_t* vertex_cluster, int64_t* counts_dev, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = sg_counts_check("perf_meshsimp_cluster", n_vertices, n_faces)) return rc;
    SgGrid grid;
    if (int rc = sg_grid_check("perf_meshsimp_cluster", lo, h, nx, ny, nz, &grid)) return rc;
    PERF_REQUIRE(vertices || n_vertices == 0, "perf_meshsimp_cluster: NULL input (vertices) with vertices to cluster");
    PERF_REQUIRE(vertex_cluster || n_vertices == 0, "perf_meshsimp_cluster: NULL output (vertex_cluster) with vertices to cluster");
    PERF_REQUIRE(counts_dev, "perf_meshsimp_cluster: NULL output (counts_dev)");
    if (int rc = sg_workspace_check("perf_meshsimp_cluster", n_vertices, n_faces, workspace, workspace_bytes)) return rc;
    const SgLayout l = sg_layout(workspace, n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    const int bits = sg_table_bits(n_vertices);
    bool ok = hipMemsetAsync(l.totals, 0xff, 4 * sizeof(int64_t), st) == hipSuccess;          // the flag: no bad vertex (-1, the largest unsigned)
    if (n_vertices > 0) ok = ok && hipMemsetAsync(l.vtable, 0xff, sizeof(uint32_t) << bits, st) == hipSuccess;          // EMPTY
    if (!ok) {
        (void)hipGetLastError();
        set_error("perf_meshsimp_cluster: clearing the table failed");
        return PERF_E_LAUNCH;
    }
    const uint64_t* total = nullptr;
    if (n_vertices > 0) {
        const unsigned groups = scan_groups(n_vertices);
        hipLaunchKernelGGL(meshsimp_keys_kernel, dim3(groups), dim3(kSgGroup), 0, st, vertices, n_vertices, grid, l.keys, (unsigned long long*)(l.totals + 1));
        hipLaunchKernelGGL(meshsimp_insert_cells_kernel, dim3(groups), dim3(kSgGroup), 0, st, (const int64_t*)l.keys, n_vertices, l.vtable, bits, l.slot);
        hipLaunchKernelGGL(meshsimp_smallest_kernel, dim3(groups), dim3(kSgGroup), 0, st, (const int64_t*)l.keys, (const uint32_t*)l.vtable, n_vertices, l.slot,
                           l.smallest, l.vsums);
        total = scan_u64(l.vsums, groups, l.vsums + groups, st);
        hipLaunchKernelGGL(meshsimp_ids_kernel, dim3(groups), dim3(kSgGroup), 0, st, (const int32_t*)l.smallest, (const uint32_t*)l.slot, (const uint64_t*)l.vsums,
                           n_vertices, vertex_cluster);
    }
    hipLaunchKernelGGL(meshsimp_totals_kernel, dim3(1), dim3(64), 0, st, total, l.totals, counts_dev);
    PERF_LAUNCH_CHECK("perf_meshsimp_cluster");
    return PERF_OK;
}

extern "C" int perf_meshsimp_place(const float* vertices, int64_t n_vertices, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz,
                                   const int32_t* vertex_cluster, int64_t n_clusters, int32_t placement, float* cluster_vertices, int32_t* representative,
                                   void* scratch, int64_t scratch_bytes, void* stream) {
    if (int rc = sg_counts_check("perf_meshsimp_place", n_vertices, 0)) return rc;
    SgGrid grid;
    if (int rc = sg_grid_check("perf_meshsimp_place", lo, h, nx, ny, nz, &grid)) return rc;
    PERF_REQUIRE(n_clusters >= 0, "perf_meshsimp_place: a negative number of clusters (%lld)", (long long)n_clusters);
    PERF_REQUIRE(n_clusters <= n_vertices, "perf_meshsimp_place: %lld clusters, the mesh has %lld vertices", (long long)n_clusters, (long long)n_vertices);
    PERF_REQUIRE(placement == PERF_MESHSIMP_PLACE_MEAN || placement == PERF_MESHSIMP_PLACE_MEMBER, "perf_meshsimp_place: placement %d is neither mean (0) nor member (1)",
                 (int)placement);
    PERF_REQUIRE((vertices && vertex_cluster) || n_vertices == 0, "perf_meshsimp_place: NULL input (vertices or vertex_cluster) with vertices to place");
    PERF_REQUIRE((cluster_vertices && representative) || n_clusters == 0, "perf_meshsimp_place: NULL output (cluster_vertices or representative) with clusters to place");
    PERF_REQUIRE(scratch || n_clusters == 0, "perf_meshsimp_place: NULL workspace (scratch) with clusters to place");
    PERF_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "perf_meshsimp_place: the scratch must be 16-byte aligned");
    PERF_REQUIRE(scratch_bytes >= 48 * n_clusters, "perf_meshsimp_place: the scratch holds %lld bytes, %lld are needed", (long long)scratch_bytes,
                 (long long)(48 * n_clusters));
    if (n_clusters == 0) return PERF_OK;
    const SgScratch s = sg_scratch(scratch, n_clusters);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(s.sums, 0, 5 * n_clusters * sizeof(int64_t), st) != hipSuccess || hipMemsetAsync(s.best, 0xff, n_clusters * sizeof(int64_t), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_meshsimp_place: clearing the scratch failed");
        return PERF_E_LAUNCH;
    }
    const unsigned vgroups = scan_groups(n_vertices), cgroups = scan_groups(n_clusters), pgroups = (unsigned)div_up(n_vertices, kSgPlaceGroup);
    hipLaunchKernelGGL(meshsimp_sums_kernel, dim3(pgroups), dim3(kSgPlaceGroup), 0, st, vertices, n_vertices, grid, vertex_cluster, n_clusters, s);
    hipLaunchKernelGGL(meshsimp_mean_kernel, dim3(cgroups), dim3(kSgGroup), 0, st, grid, n_clusters, s, placement, cluster_vertices, representative);
    hipLaunchKernelGGL(meshsimp_nearest_kernel, dim3(pgroups), dim3(kSgPlaceGroup), 0, st, vertices, n_vertices, vertex_cluster, n_clusters, s);
    hipLaunchKernelGGL(meshsimp_representative_kernel, dim3(vgroups), dim3(kSgGroup), 0, st, vertices, n_vertices, vertex_cluster, n_clusters, s, representative);
    hipLaunchKernelGGL(meshsimp_finish_kernel, dim3(cgroups), dim3(kSgGroup), 0, st, vertices, n_vertices, n_clusters, placement, cluster_vertices, representative);
    PERF_LAUNCH_CHECK("perf_meshsimp_place");
    return PERF_OK;
}

extern "C" int perf_meshsimp_faces(const int32_t* faces, int64_t n_faces, const int32_t* vertex_cluster, int64_t n_vertices, int32_t dedupe, int32_t* faces_out,
                                   uint8_t* face_keep, int64_t* bad_face_dev, void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = sg_counts_check("perf_meshsimp_faces", n_vertices, n_faces)) return rc;
    PERF_REQUIRE(dedupe == PERF_MESHSIMP_DEDUPE_NONE || dedupe == PERF_MESHSIMP_DEDUPE_ORIENTED || dedupe == PERF_MESHSIMP_DEDUPE_UNORIENTED,
                 "perf_meshsimp_faces: dedupe %d is none of none (0), oriented (1), unoriented (2)", (int)dedupe);
    PERF_REQUIRE(faces || n_faces == 0, "perf_meshsimp_faces: NULL input (faces) with faces to follow");
    PERF_REQUIRE(vertex_cluster || n_vertices == 0, "perf_meshsimp_faces: NULL input (vertex_cluster) with vertices");
    PERF_REQUIRE((faces_out && face_keep) || n_faces == 0, "perf_meshsimp_faces: NULL output (faces_out or face_keep) with faces to follow");
    PERF_REQUIRE(bad_face_dev, "perf_meshsimp_faces: NULL output (bad_face_dev)");
    if (int rc = sg_workspace_check("perf_meshsimp_faces", n_vertices, n_faces, workspace, workspace_bytes)) return rc;
    const SgLayout l = sg_layout(workspace, n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    const int bits = sg_table_bits(n_faces);
    bool ok = hipMemsetAsync(bad_face_dev, 0xff, sizeof(int64_t), st) == hipSuccess;          // no bad face (-1, the largest unsigned)
    if (n_faces > 0 && dedupe != PERF_MESHSIMP_DEDUPE_NONE) ok = ok && hipMemsetAsync(l.ftable, 0xff, sizeof(uint32_t) << bits, st) == hipSuccess;          // EMPTY
    if (!ok) {
        (void)hipGetLastError();
        set_error("perf_meshsimp_faces: clearing the table failed");
        return PERF_E_LAUNCH;
    }
    if (n_faces > 0) {
        const unsigned groups = scan_groups(n_faces);
        hipLaunchKernelGGL(meshsimp_remap_kernel, dim3(groups), dim3(kSgGroup), 0, st, faces, n_faces, vertex_cluster, n_vertices, faces_out, face_keep,
                           (unsigned long long*)bad_face_dev);
        if (dedupe == PERF_MESHSIMP_DEDUPE_ORIENTED)
            hipLaunchKernelGGL(meshsimp_insert_faces_kernel<false>, dim3(groups), dim3(kSgGroup), 0, st, (const int32_t*)faces_out, (const uint8_t*)face_keep, n_faces,
                               l.ftable, bits, l.fslot);
        if (dedupe == PERF_MESHSIMP_DEDUPE_UNORIENTED)
            hipLaunchKernelGGL(meshsimp_insert_faces_kernel<true>, dim3(groups), dim3(kSgGroup), 0, st, (const int32_t*)faces_out, (const uint8_t*)face_keep, n_faces,
                               l.ftable, bits, l.fslot);
        if (dedupe != PERF_MESHSIMP_DEDUPE_NONE)
            hipLaunchKernelGGL(meshsimp_resolve_kernel, dim3(groups), dim3(kSgGroup), 0, st, (const uint32_t*)l.ftable, (const uint32_t*)l.fslot, n_faces, face_keep);
    }
    PERF_LAUNCH_CHECK("perf_meshsimp_faces");
    return PERF_OK;
}
