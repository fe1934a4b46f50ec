// Connected components of a triangle mesh (include/perf_hip_meshcc.h): init -> hook -> roots -> smallest -> rank -> scan -> ids; stats; filter
// count -> scan -> write.  The hook is a wait-free union-find in ONE launch: parents only fall, a failed compare-and-swap goes on from
// the value it returned, every read of a parent is an agent-scope relaxed atomic load (the header has the termination argument).
// The roots' launch jumps pointers the same way; everything after it reads what an ended launch wrote, with plain loads.
#include "common.hpp"
#include "mesh_filter_device.hpp"
#include "../../include/perf_hip_meshcc.h"

namespace perf {

constexpr int kCcGroup = kScanGroup;         // items of one workgroup: one per thread (group_rank's workgroup)
constexpr int kCcPerThread = 16;             // stats, smallest: items one thread takes before the workgroup's flush

struct CcLayout {
    int32_t* a;              // [V] the parents' keys; then each root's smallest vertex; then the ranks within their groups of the components'
                             // smallest vertices; in the filter the kept vertices' new indices
    int32_t* b;              // [V] roots, then the components' smallest vertices
    uint64_t* vsums;         // S(V)
    uint64_t* fsums;         // S(F)
    int64_t* totals;         // [4] label: (C, first bad face); filter: (V', F')
};

static inline CcLayout cc_layout(void* workspace, int64_t n_vertices, int64_t n_faces) {
    CcLayout l;
    l.a = (int32_t*)workspace;
    l.b = l.a + n_vertices;
    l.vsums = (uint64_t*)workspace + n_vertices;
    l.fsums = l.vsums + group_words(n_vertices);
    l.totals = (int64_t*)(l.fsums + group_words(n_faces));
    return l;
}

// ---- label ------------------------------------------------------------------------------------------------------------------------------
// The order the forest is built in: vertex x comes before y when key(x) < key(y), key a bijection of the 32-bit words that scatters
// neighbouring indices (two odd multiplications around a shift-xor; unkey inverts it).  Hooking by INDEX would turn a strip of a mesh
// whose indices ascend along it -- every surface-nets mesh -- into one chain as long as the strip when all its faces hook at once.
constexpr uint32_t kCcMulA = 0x9E3779B1u, kCcMulB = 0x85EBCA6Bu;
constexpr uint32_t cc_inverse(uint32_t a) {                 // of an odd a modulo 2^32 (Newton: the correct bits double per step)
    uint32_t x = a;
    for (int i = 0; i < 5; ++i) x *= 2u - a * x;
    return x;
}
constexpr uint32_t kCcInvA = cc_inverse(kCcMulA), kCcInvB = cc_inverse(kCcMulB);
static_assert(kCcMulA * kCcInvA == 1u && kCcMulB * kCcInvB == 1u, "modular inverses");
__host__ __device__ constexpr uint32_t cc_key(uint32_t v) {
    uint32_t k = v * kCcMulA;
    k ^= k >> 16;
    return k * kCcMulB;
}
__host__ __device__ constexpr uint32_t cc_unkey(uint32_t k) {
    k *= kCcInvB;
    k ^= k >> 16;
    return k * kCcInvA;
}
static_assert(cc_unkey(cc_key(0u)) == 0u && cc_unkey(cc_key(12345u)) == 12345u && cc_unkey(cc_key(0x3fffffffu)) == 0x3fffffffu, "unkey inverts key");

// parent[x] holds the KEY of x's parent: only keys of vertices of the mesh are ever stored, so unkey of a stored word indexes in bounds
__global__ void __launch_bounds__(kCcGroup) meshcc_init_kernel(uint32_t* __restrict__ parent, int64_t n_vertices) {
    const int64_t v = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    if (v < n_vertices) parent[v] = cc_key((uint32_t)v);
}

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Joins the trees of the vertices with keys a and b.  Only the HIGHER of the two ends climbs, so the ends meet at their first common
// ancestor when they are in one tree already -- the root's own word, which every walk of a big component would end on, is never read --
// and otherwise the higher end arrives at a root, which is hung below the other end (any vertex before it in the order will do).
// INVARIANT: {u, v} = {an ancestor-or-self of a, one of b}, so what is left in v at the end is an ancestor of both, and a and b take it
// for their parent: atomicMin on their own words, which keeps parents falling under any race and touches no root (a vertex with a proper
// ancestor is none).  Every step replaces the higher end by a value below it -- read from its parent's word, or RETURNED by the failed
// compare-and-swap -- so the loop ends after fewer than 2 V steps whatever the other threads do.
__device__ __forceinline__ void cc_union(uint32_t* parent, uint32_t a, uint32_t b) {
    uint32_t u = a, v = b;
    int steps = 0;
    while (u != v) {
        if (u < v) { const uint32_t t = u; u = v; v = t; }
        uint32_t p = cc_load(parent + cc_unkey(u));
        if (p == u) {                                       // u looks like a root: hang it below v
            p = atomicCAS(parent + cc_unkey(u), u, v);
            if (p == u) break;                              // it was one
        }
        u = p;                                              // p < u: the parent of u as loaded, or as the compare-and-swap returned it
        ++steps;
    }
    if (steps >= 2) {                                       // (after fewer steps a and b are at most one hop from it)
        if (a != v) atomicMin(parent + cc_unkey(a), v);
        if (b != v) atomicMin(parent + cc_unkey(b), v);
    }
}

__global__ void __launch_bounds__(kCcGroup) meshcc_hook_kernel(const int32_t* __restrict__ faces, int64_t n_faces, int64_t n_vertices, uint32_t* parent,
                                                               unsigned long long* __restrict__ first_bad) {
    const int64_t f = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const bool good = a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices;
    if (!good) {
        atomicMin(first_bad, (unsigned long long)f);
        return;
    }
    if (a != b) cc_union(parent, cc_key((uint32_t)a), cc_key((uint32_t)b));
    if (b != c && a != c) cc_union(parent, cc_key((uint32_t)b), cc_key((uint32_t)c));          // (a == c: (a, b) said it all)
}

// After the hook's launch no root changes any more.  Vertex v walks to its root and moves ITS OWN parent along as it goes (only thread v
// stores parent[v], each value an ancestor below the last), so a walk that passes through v skips what v has already passed: pointer
// jumping without rounds.  p falls with every step, whatever the other threads do and however stale a read is.  -> the root's INDEX
__global__ void __launch_bounds__(kCcGroup) meshcc_roots_kernel(uint32_t* parent, int64_t n_vertices, int32_t* __restrict__ roots) {
    const int64_t v = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    if (v >= n_vertices) return;
    uint32_t p = cc_load(parent + v);
    if (p != cc_key((uint32_t)v)) {
        uint32_t g = cc_load(parent + cc_unkey(p));
        while (g != p) {                                    // g < p
            __hip_atomic_store(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            p = g;
            g = cc_load(parent + cc_unkey(p));
        }
    }
    roots[v] = (int32_t)cc_unkey(p);
}

// What the threads of a workgroup hold per component -- a count and a volume to add, or (kMin) an index to take the minimum of -- goes
// out once per wave and distinct component, and the waves' first components once per workgroup where they agree: a mesh is mostly ONE
// component, and every atomic on its word is served in turn.  All 256 threads arrive.
template <bool kMin>
__device__ __forceinline__ void cc_emit(int32_t c, long long n, double s, unsigned long long* __restrict__ counts64, int32_t* __restrict__ counts32,
                                        double* __restrict__ volumes) {
    if (kMin) {
        atomicMin(counts32 + c, (int32_t)n);
    } else {
        if (counts64) atomicAdd(counts64 + c, (unsigned long long)n);
        if (counts32) atomicAdd(counts32 + c, (int32_t)n);
        if (volumes) unsafeAtomicAdd(volumes + c, s);
    }
}

template <bool kMin>
__device__ __forceinline__ void cc_block_flush(bool has, int32_t comp, long long count, double volume, unsigned long long* __restrict__ counts64,
                                               int32_t* __restrict__ counts32, double* __restrict__ volumes) {
    __shared__ int32_t first_comp[kCcGroup / 64];
    __shared__ long long first_count[kCcGroup / 64];
    __shared__ double first_volume[kCcGroup / 64];
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) first_comp[wave] = -1;
    uint64_t todo = __ballot(has);
    bool first = true;
    while (todo) {                                          // (wave-uniform)
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int32_t c = __shfl(comp, leader);
        const bool mine = has && comp == c;
        todo &= ~__ballot(mine);
        long long n = mine ? count : (kMin ? 0x7fffffffffffffffll : 0ll);
        double s = mine ? volume : 0.0;
        for (int off = 32; off > 0; off >>= 1) {
            const long long other = __shfl_xor(n, off);
            n = kMin ? (other < n ? other : n) : n + other;
            if (!kMin) s += __shfl_xor(s, off);
        }
        if (lane == leader) {
            if (first) { first_comp[wave] = c; first_count[wave] = n; first_volume[wave] = s; }
            else cc_emit<kMin>(c, n, s, counts64, counts32, volumes);
        }
        first = false;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 0; w < kCcGroup / 64; ++w) {
        const int32_t c = first_comp[w];
        if (c < 0) continue;
        long long n = first_count[w];
        double s = first_volume[w];
        for (int u = w + 1; u < kCcGroup / 64; ++u)
            if (first_comp[u] == c) {
                n = kMin ? (first_count[u] < n ? first_count[u] : n) : n + first_count[u];
                s += first_volume[u];
                first_comp[u] = -1;
            }
        cc_emit<kMin>(c, n, s, counts64, counts32, volumes);
    }
}

// smallest[r] (set to a word above every index before the launch) = the smallest vertex of root r's tree.  A workgroup takes 256 * 16
// consecutive vertices, a thread every 256th of them; a thread keeps the run of vertices of one root (the run's first is its smallest).
__global__ void __launch_bounds__(kCcGroup) meshcc_smallest_kernel(const int32_t* __restrict__ roots, int64_t n_vertices, int32_t* __restrict__ smallest) {
    const int64_t base = (int64_t)blockIdx.x * (kCcGroup * kCcPerThread) + threadIdx.x;
    int32_t run = -1;
    long long low = 0;
    for (int k = 0; k < kCcPerThread; ++k) {
        const int64_t v = base + (int64_t)k * kCcGroup;
        if (v >= n_vertices) break;
        const int32_t r = roots[v];                         // a vertex: what the roots' launch wrote
        if (r != run) {
            if (run >= 0) atomicMin(smallest + run, (int32_t)low);
            run = r; low = v;
        }
    }
    cc_block_flush<true>(run >= 0, run, low, 0.0, nullptr, smallest, nullptr);
}

// roots[v] = the smallest vertex of v's component from here on
__global__ void __launch_bounds__(kCcGroup) meshcc_canon_kernel(int32_t* __restrict__ roots, const int32_t* __restrict__ smallest, int64_t n_vertices) {
    const int64_t v = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    if (v >= n_vertices) return;
    const int32_t s = smallest[roots[v]];
    roots[v] = s >= 0 && s <= v ? s : (int32_t)v;           // (s is in [0, v]: v itself took part in the minimum)
}

// rank[v]: the rank of vertex v among the smallest vertices of its group (smallest's array is free now); the group's count to sums
__global__ void __launch_bounds__(kCcGroup) meshcc_root_rank_kernel(const int32_t* __restrict__ roots, int64_t n_vertices, int32_t* __restrict__ rank,
                                                                    uint64_t* __restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    const bool is_root = v < n_vertices && roots[v] == (int32_t)v;
    const int32_t r = group_rank(is_root, sums);
    if (v < n_vertices) rank[v] = r;
}

__global__ void __launch_bounds__(kCcGroup) meshcc_ids_kernel(const int32_t* __restrict__ roots, const int32_t* __restrict__ rank,
                                                              const uint64_t* __restrict__ prefix, int64_t n_vertices, int32_t* __restrict__ vertex_component) {
    const int64_t v = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    if (v >= n_vertices) return;
    const int32_t r = roots[v];                             // in [0, v]
    vertex_component[v] = (int32_t)prefix[r / kCcGroup] + rank[r];
}

// (first, second) of the totals, to the workspace and to the caller
__global__ void meshcc_totals_kernel(const uint64_t* __restrict__ first, const uint64_t* __restrict__ second, bool keep_second, int64_t* __restrict__ totals,
                                     int64_t* __restrict__ counts_dev) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t a = first ? (int64_t)first[0] : 0;
    const int64_t b = keep_second ? totals[1] : (second ? (int64_t)second[0] : 0);
    totals[0] = a; totals[1] = b; totals[2] = 0; totals[3] = 0;
    counts_dev[0] = a; counts_dev[1] = b;
}

// ---- stats ------------------------------------------------------------------------------------------------------------------------------
// A workgroup takes 256 * 16 consecutive faces, a thread every 256th of them; a thread sums the run of faces of one component and
// adds it on its own only where the component changes under it.
__global__ void __launch_bounds__(kCcGroup) meshcc_face_stats_kernel(const int32_t* __restrict__ faces, int64_t n_faces, const float* __restrict__ vertices,
                                                                     int64_t n_vertices, const int32_t* __restrict__ vertex_component, int64_t n_components,
                                                                     unsigned long long* __restrict__ faces_per, double* __restrict__ volumes) {
    const int64_t base = (int64_t)blockIdx.x * (kCcGroup * kCcPerThread) + threadIdx.x;
    int32_t run = -1;
    long long count = 0;
    double volume = 0.0;
    for (int k = 0; k < kCcPerThread; ++k) {
        const int64_t f = base + (int64_t)k * kCcGroup;
        if (f >= n_faces) break;
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (!(a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices)) continue;
        const int32_t comp = vertex_component[a];
        if (comp < 0 || comp >= n_components) continue;
        if (comp != run) {
            if (run >= 0) cc_emit<false>(run, count, volume, faces_per, nullptr, volumes);
            run = comp; count = 0; volume = 0.0;
        }
        ++count;
        if (volumes) {
            const double ax = vertices[3 * (int64_t)a], ay = vertices[3 * (int64_t)a + 1], az = vertices[3 * (int64_t)a + 2];
            const double bx = vertices[3 * (int64_t)b], by = vertices[3 * (int64_t)b + 1], bz = vertices[3 * (int64_t)b + 2];
            const double cx = vertices[3 * (int64_t)c], cy = vertices[3 * (int64_t)c + 1], cz = vertices[3 * (int64_t)c + 2];
            volume += (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)) / 6.0;
        }
    }
    cc_block_flush<false>(run >= 0, run, count, volume, faces_per, nullptr, volumes);
}

__global__ void __launch_bounds__(kCcGroup) meshcc_vertex_stats_kernel(const int32_t* __restrict__ vertex_component, int64_t n_vertices, int64_t n_components,
                                                                       int32_t* __restrict__ vertices_per) {
    const int64_t base = (int64_t)blockIdx.x * (kCcGroup * kCcPerThread) + threadIdx.x;
    int32_t run = -1;
    long long count = 0;
    for (int k = 0; k < kCcPerThread; ++k) {
        const int64_t v = base + (int64_t)k * kCcGroup;
        if (v >= n_vertices) break;
        const int32_t comp = vertex_component[v];
        if (comp < 0 || comp >= n_components) continue;
        if (comp != run) {
            if (run >= 0) atomicAdd(vertices_per + run, (int32_t)count);
            run = comp; count = 0;
        }
        ++count;
    }
    cc_block_flush<false>(run >= 0, run, count, 0.0, nullptr, vertices_per, nullptr);
}

// ---- filter (the compaction is mesh_filter_device.hpp's, by the two predicates below) -----------------------------------------------------
__device__ __forceinline__ bool cc_vertex_kept(const int32_t* __restrict__ vertex_component, const uint8_t* __restrict__ keep, int64_t n_vertices,
                                               int64_t n_components, int64_t v) {
    if (v < 0 || v >= n_vertices) return false;
    const int32_t comp = vertex_component[v];
    return comp >= 0 && comp < n_components && keep[comp] != 0;
}

// a face is kept iff its three indices are vertices and the first one's component is kept (all three share it)
__device__ __forceinline__ bool cc_face_kept(const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_component, const uint8_t* __restrict__ keep,
                                             int64_t n_faces, int64_t n_vertices, int64_t n_components, int64_t f, int32_t abc[3]) {
    if (f >= n_faces) return false;
    abc[0] = faces[3 * f]; abc[1] = faces[3 * f + 1]; abc[2] = faces[3 * f + 2];
    if (!(abc[0] >= 0 && abc[0] < n_vertices && abc[1] >= 0 && abc[1] < n_vertices && abc[2] >= 0 && abc[2] < n_vertices)) return false;
    return cc_vertex_kept(vertex_component, keep, n_vertices, n_components, abc[0]);
}

struct CcVertexKept {
    const int32_t* vertex_component;
    const uint8_t* keep;
    int64_t n_vertices, n_components;
    __device__ __forceinline__ bool operator()(int64_t v) const { return cc_vertex_kept(vertex_component, keep, n_vertices, n_components, v); }
};

struct CcFaceKept {
    const int32_t* faces;
    const int32_t* vertex_component;
    const uint8_t* keep;
    int64_t n_faces, n_vertices, n_components;
    __device__ __forceinline__ bool operator()(int64_t f, int32_t abc[3]) const {
        return cc_face_kept(faces, vertex_component, keep, n_faces, n_vertices, n_components, f, abc);
    }
};

__global__ void __launch_bounds__(kCcGroup) meshcc_keep_vertices_kernel(const int32_t* __restrict__ vertex_component, const uint8_t* __restrict__ keep,
                                                                        int64_t n_vertices, int64_t n_components, uint64_t* __restrict__ sums) {
    const int64_t v = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    group_rank(cc_vertex_kept(vertex_component, keep, n_vertices, n_components, v), sums);
}

__global__ void __launch_bounds__(kCcGroup) meshcc_keep_faces_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ vertex_component,
                                                                     const uint8_t* __restrict__ keep, int64_t n_faces, int64_t n_vertices, int64_t n_components,
                                                                     uint64_t* __restrict__ sums) {
    const int64_t f = (int64_t)blockIdx.x * kCcGroup + threadIdx.x;
    int32_t abc[3];
    group_rank(cc_face_kept(faces, vertex_component, keep, n_faces, n_vertices, n_components, f, abc), sums);
}

// ---- the checks of the entry points -------------------------------------------------------------------------------------------------------
static int cc_counts_check(const char* who, int64_t n_vertices, int64_t n_faces) {
    return mesh_counts_check(who, n_vertices, n_faces, PERF_MESHCC_MAX_VERTICES, PERF_MESHCC_MAX_FACES, "2^38");
}

static int cc_components_check(const char* who, int64_t n_components, int64_t n_vertices) {
    PERF_REQUIRE(n_components >= 0, "%s: a negative number of components (%lld)", who, (long long)n_components);
    PERF_REQUIRE(n_components <= n_vertices, "%s: %lld components, the mesh has %lld vertices", who, (long long)n_components, (long long)n_vertices);
    return PERF_OK;
}

static int cc_workspace_check(const char* who, int64_t n_vertices, int64_t n_faces, const void* workspace, int64_t workspace_bytes) {
    return workspace_check(who, perf_meshcc_workspace_bytes(n_vertices, n_faces), workspace, workspace_bytes);
}

}  // namespace perf

using namespace perf;

extern "C" int perf_meshcc_version(void) { return PERF_MESHCC_ABI_VERSION; }

extern "C" int64_t perf_meshcc_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (cc_counts_check("perf_meshcc_workspace_bytes", n_vertices, n_faces) != PERF_OK) return -1;
    const int64_t words = n_vertices + group_words(n_vertices) + group_words(n_faces) + 4;
    return ((words + 1) & ~(int64_t)1) * (int64_t)sizeof(uint64_t);      // (a multiple of 16)
}

extern "C" int perf_meshcc_label(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* vertex_component, int64_t* counts_dev,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    if (int rc = cc_counts_check("perf_meshcc_label", n_vertices, n_faces)) return rc;
    PERF_REQUIRE(faces || n_faces == 0, "perf_meshcc_label: NULL input (faces) with faces to follow");
    PERF_REQUIRE(vertex_component || n_vertices == 0, "perf_meshcc_label: NULL output (vertex_component) with vertices to label");
    PERF_REQUIRE(counts_dev, "perf_meshcc_label: NULL output (counts_dev)");
    if (int rc = cc_workspace_check("perf_meshcc_label", n_vertices, n_faces, workspace, workspace_bytes)) return rc;
    const CcLayout l = cc_layout(workspace, n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(l.totals, 0xff, 4 * sizeof(int64_t), st) != hipSuccess) {          // the flag: no bad face (-1, the largest unsigned)
        (void)hipGetLastError();
        set_error("perf_meshcc_label: clearing the totals failed");
        return PERF_E_LAUNCH;
    }
    const uint64_t* total = nullptr;
    if (n_vertices > 0) {
        const unsigned groups = scan_groups(n_vertices);
        hipLaunchKernelGGL(meshcc_init_kernel, dim3(groups), dim3(kCcGroup), 0, st, (uint32_t*)l.a, n_vertices);
        if (n_faces > 0)
            hipLaunchKernelGGL(meshcc_hook_kernel, dim3(scan_groups(n_faces)), dim3(kCcGroup), 0, st, faces, n_faces, n_vertices, (uint32_t*)l.a,
                               (unsigned long long*)(l.totals + 1));
        hipLaunchKernelGGL(meshcc_roots_kernel, dim3(groups), dim3(kCcGroup), 0, st, (uint32_t*)l.a, n_vertices, l.b);
        if (hipMemsetAsync(l.a, 0x7f, n_vertices * sizeof(int32_t), st) != hipSuccess) {          // 0x7f7f7f7f: above every index
            (void)hipGetLastError();
            set_error("perf_meshcc_label: clearing the smallest vertices failed");
            return PERF_E_LAUNCH;
        }
        hipLaunchKernelGGL(meshcc_smallest_kernel, dim3((unsigned)div_up(n_vertices, kCcGroup * kCcPerThread)), dim3(kCcGroup), 0, st, (const int32_t*)l.b, n_vertices, l.a);
        hipLaunchKernelGGL(meshcc_canon_kernel, dim3(groups), dim3(kCcGroup), 0, st, l.b, (const int32_t*)l.a, n_vertices);
        hipLaunchKernelGGL(meshcc_root_rank_kernel, dim3(groups), dim3(kCcGroup), 0, st, (const int32_t*)l.b, n_vertices, l.a, l.vsums);
        total = scan_u64(l.vsums, groups, l.vsums + groups, st);
        hipLaunchKernelGGL(meshcc_ids_kernel, dim3(groups), dim3(kCcGroup), 0, st, (const int32_t*)l.b, (const int32_t*)l.a, (const uint64_t*)l.vsums, n_vertices,
                           vertex_component);
    } else if (n_faces > 0) {                               // every face is out of range: the first one is the first bad one
        hipLaunchKernelGGL(meshcc_hook_kernel, dim3(1), dim3(kCcGroup), 0, st, faces, (int64_t)1, n_vertices, (uint32_t*)nullptr,
                           (unsigned long long*)(l.totals + 1));
    }
    hipLaunchKernelGGL(meshcc_totals_kernel, dim3(1), dim3(64), 0, st, total, (const uint64_t*)nullptr, true, l.totals, counts_dev);
    PERF_LAUNCH_CHECK("perf_meshcc_label");
    return PERF_OK;
}

extern "C" int perf_meshcc_stats(const int32_t* faces, int64_t n_faces, const float* vertices, int64_t n_vertices, const int32_t* vertex_component,
                                 int64_t n_components, int64_t* faces_per_component, int32_t* vertices_per_component, double* signed_volume, void* stream) {
    if (int rc = cc_counts_check("perf_meshcc_stats", n_vertices, n_faces)) return rc;
    if (int rc = cc_components_check("perf_meshcc_stats", n_components, n_vertices)) return rc;
    PERF_REQUIRE(faces || n_faces == 0, "perf_meshcc_stats: NULL input (faces) with faces to count");
    PERF_REQUIRE(vertex_component || n_vertices == 0, "perf_meshcc_stats: NULL input (vertex_component) with vertices to count");
    PERF_REQUIRE((faces_per_component && vertices_per_component) || n_components == 0,
                 "perf_meshcc_stats: NULL output (faces_per_component or vertices_per_component) with components to fill");
    PERF_REQUIRE(signed_volume || !vertices || n_components == 0, "perf_meshcc_stats: NULL output (signed_volume) with vertices given");
    if (n_components == 0) return PERF_OK;
    hipStream_t st = as_stream(stream);
    bool ok = hipMemsetAsync(faces_per_component, 0, n_components * sizeof(int64_t), st) == hipSuccess;
    ok = ok && hipMemsetAsync(vertices_per_component, 0, n_components * sizeof(int32_t), st) == hipSuccess;
    if (signed_volume) ok = ok && hipMemsetAsync(signed_volume, 0, n_components * sizeof(double), st) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        set_error("perf_meshcc_stats: clearing the outputs failed");
        return PERF_E_LAUNCH;
    }
    if (n_faces > 0)
        hipLaunchKernelGGL(meshcc_face_stats_kernel, dim3((unsigned)div_up(n_faces, kCcGroup * kCcPerThread)), dim3(kCcGroup), 0, st, faces, n_faces, vertices,
                           n_vertices, vertex_component, n_components, (unsigned long long*)faces_per_component, vertices ? signed_volume : (double*)nullptr);
    hipLaunchKernelGGL(meshcc_vertex_stats_kernel, dim3((unsigned)div_up(n_vertices, kCcGroup * kCcPerThread)), dim3(kCcGroup), 0, st, vertex_component, n_vertices, n_components,
                       vertices_per_component);
    PERF_LAUNCH_CHECK("perf_meshcc_stats");
    return PERF_OK;
}

static int cc_filter_check(const char* who, const int32_t* faces, int64_t n_faces, const int32_t* vertex_component, int64_t n_vertices, const uint8_t* keep,
                           int64_t n_components, const void* workspace, int64_t workspace_bytes) {
    if (int rc = cc_counts_check(who, n_vertices, n_faces)) return rc;
    if (int rc = cc_components_check(who, n_components, n_vertices)) return rc;
    PERF_REQUIRE(faces || n_faces == 0, "%s: NULL input (faces) with faces to filter", who);
    PERF_REQUIRE(vertex_component || n_vertices == 0, "%s: NULL input (vertex_component) with vertices to filter", who);
    PERF_REQUIRE(keep || n_components == 0, "%s: NULL input (keep) with components to select", who);
    return cc_workspace_check(who, n_vertices, n_faces, workspace, workspace_bytes);
}

extern "C" int perf_meshcc_filter_count(const int32_t* faces, int64_t n_faces, const int32_t* vertex_component, int64_t n_vertices, const uint8_t* keep,
                                        int64_t n_components, void* workspace, int64_t workspace_bytes, int64_t* counts_dev, void* stream) {
    if (int rc = cc_filter_check("perf_meshcc_filter_count", faces, n_faces, vertex_component, n_vertices, keep, n_components, workspace, workspace_bytes)) return rc;
    PERF_REQUIRE(counts_dev, "perf_meshcc_filter_count: NULL output (counts_dev)");
    const CcLayout l = cc_layout(workspace, n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    const uint64_t *v_total = nullptr, *f_total = nullptr;
    if (n_vertices > 0) {
        const unsigned groups = scan_groups(n_vertices);
        hipLaunchKernelGGL(meshcc_keep_vertices_kernel, dim3(groups), dim3(kCcGroup), 0, st, vertex_component, keep, n_vertices, n_components, l.vsums);
        v_total = scan_u64(l.vsums, groups, l.vsums + groups, st);
        hipLaunchKernelGGL(filter_new_index_kernel<CcVertexKept>, dim3(groups), dim3(kCcGroup), 0, st, CcVertexKept{vertex_component, keep, n_vertices, n_components},
                           (const uint64_t*)l.vsums, l.a);
    }
    if (n_faces > 0) {
        const unsigned groups = scan_groups(n_faces);
        hipLaunchKernelGGL(meshcc_keep_faces_kernel, dim3(groups), dim3(kCcGroup), 0, st, faces, vertex_component, keep, n_faces, n_vertices, n_components, l.fsums);
        f_total = scan_u64(l.fsums, groups, l.fsums + groups, st);
    }
    hipLaunchKernelGGL(meshcc_totals_kernel, dim3(1), dim3(64), 0, st, v_total, f_total, false, l.totals, counts_dev);
    PERF_LAUNCH_CHECK("perf_meshcc_filter_count");
    return PERF_OK;
}

extern "C" int perf_meshcc_filter_write(const int32_t* faces, int64_t n_faces, const int32_t* vertex_component, int64_t n_vertices, const uint8_t* keep,
                                        int64_t n_components, const float* vertices, const void* workspace, int64_t workspace_bytes, float* vertices_out,
                                        int32_t* kept_vertex_index, int64_t vertex_capacity, int32_t* faces_out, int64_t face_capacity, void* stream) {
    if (int rc = cc_filter_check("perf_meshcc_filter_write", faces, n_faces, vertex_component, n_vertices, keep, n_components, workspace, workspace_bytes)) return rc;
    PERF_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, "perf_meshcc_filter_write: negative capacity");
    PERF_REQUIRE((kept_vertex_index || vertex_capacity == 0) && (faces_out || face_capacity == 0) && (vertices_out || !vertices || vertex_capacity == 0),
                 "perf_meshcc_filter_write: NULL output with a capacity above 0");
    const CcLayout l = cc_layout(const_cast<void*>(workspace), n_vertices, n_faces);
    hipStream_t st = as_stream(stream);
    int64_t totals[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(totals, l.totals, sizeof(totals), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_meshcc_filter_write: reading the counted totals back failed");
        return PERF_E_LAUNCH;
    }
    PERF_REQUIRE(vertex_capacity >= totals[0], "perf_meshcc_filter_write: room for %lld vertices, %lld were counted", (long long)vertex_capacity, (long long)totals[0]);
    PERF_REQUIRE(face_capacity >= totals[1], "perf_meshcc_filter_write: room for %lld faces, %lld were counted", (long long)face_capacity, (long long)totals[1]);
    if (totals[0] == 0) return PERF_OK;                     // (no kept vertex: no kept face either)
    hipLaunchKernelGGL(filter_write_vertices_kernel, dim3(scan_groups(n_vertices)), dim3(kCcGroup), 0, st, (const int32_t*)l.a, n_vertices, vertices, vertices_out,
                       kept_vertex_index, vertex_capacity);
    if (totals[1] > 0)
        hipLaunchKernelGGL(filter_write_faces_kernel<CcFaceKept>, dim3(scan_groups(n_faces)), dim3(kCcGroup), 0, st,
                           CcFaceKept{faces, vertex_component, keep, n_faces, n_vertices, n_components}, (const uint64_t*)l.fsums, (const int32_t*)l.a, faces_out, face_capacity);
    PERF_LAUNCH_CHECK("perf_meshcc_filter_write");
    return PERF_OK;
}
