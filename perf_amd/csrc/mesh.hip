// Naive surface nets on a dense fp32 lattice (include/perf_hip_mesh.h): count -> scan -> write, no case tables, no atomics.
//
// A chunk is 64 cells along z of one (i, j) row, lanes along z.  The count pass needs only the corners' inside bits, so a field row of
// 64 corners is ONE coalesced load and a ballot; everything after that -- which cells are active, how many quads their edges emit -- is
// 64-bit mask arithmetic on wave-uniform values.  A wave takes kStrip consecutive j of one (i, chunk), so of the four corner rows of a
// cell row two are the previous cell row's: 2 (kStrip + 1) row loads for kStrip cell rows, all issued before the first use.  The corner
// rows of i + 1 are read again by the wave of i + 1 (through the caches); they are not staged in LDS.  The write pass touches the field
// only where a cell is active.
#include "common.hpp"
#include "mesh_device.hpp"
#include "mesh_scan_device.hpp"
#include "../../include/perf_hip_mesh.h"

namespace perf {

constexpr int kStrip = 8;            // cell rows (consecutive j) per wave of the count pass

struct MeshDims {
    int32_t nx, ny, nz, cz;          // cells per axis; chunks per row
};

static inline int64_t chunks_of(int32_t nx, int32_t ny, int32_t nz) { return (int64_t)nx * ny * div_up(nz, 64); }

__global__ void __launch_bounds__(256) mesh_count_kernel(const float* __restrict__ field, MeshDims d, float thr, int64_t n_strips, uint64_t* __restrict__ masks,
                                                         uint64_t* __restrict__ ranks) {
    const int64_t s = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (s >= n_strips) return;                      // (wave-uniform)
    const int32_t lane = threadIdx.x & 63;
    const int64_t n_jb = (d.ny + kStrip - 1) / kStrip;
    const int32_t kc = (int32_t)(s % d.cz);
    const int32_t j0 = (int32_t)((s / d.cz) % n_jb) * kStrip;
    const int32_t i = (int32_t)(s / (d.cz * n_jb));
    const int32_t k0 = kc * 64;
    const int64_t row_stride = (int64_t)d.nz + 1;
    const float* plane0 = field + (int64_t)i * (d.ny + 1) * row_stride;
    const float* plane1 = plane0 + (int64_t)(d.ny + 1) * row_stride;
    const int32_t left = d.nz - k0;                                                         // cells of this chunk: 1 .. 64 or more
    const uint64_t cells = left >= 64 ? ~0ull : ((1ull << left) - 1);
    const uint64_t k_ge1 = kc == 0 ? ~1ull : ~0ull;                                         // cells with k >= 1
    // Every load of the strip is issued before the first use: 2 (kStrip + 1) rows of 64 corners and their 65th corners, at clamped --
    // always valid -- addresses (a corner past nz, or a row past ny in the last strip, reads a neighbour that is then masked or not
    // stored).  One memory round trip per wave instead of one per cell row.
    const bool k_in = k0 + lane <= d.nz, e_in = k0 + 64 <= d.nz;
    const int32_t kk = k_in ? k0 + lane : d.nz, ke = e_in ? k0 + 64 : d.nz;
    float v0[kStrip + 1], v1[kStrip + 1], e0[kStrip + 1], e1[kStrip + 1];
#pragma unroll
    for (int r = 0; r <= kStrip; ++r) {
        const int64_t row = (int64_t)(j0 + r <= d.ny ? j0 + r : d.ny) * row_stride;
        v0[r] = plane0[row + kk]; v1[r] = plane1[row + kk];
        e0[r] = plane0[row + ke]; e1[r] = plane1[row + ke];
    }
    uint64_t a[kStrip + 1], as[kStrip + 1], b[kStrip + 1], bs[kStrip + 1];                  // rows of planes i, i+1: inside bits of corners k and k+1
#pragma unroll
    for (int r = 0; r <= kStrip; ++r) {
        a[r] = __ballot(k_in && v0[r] >= thr);
        b[r] = __ballot(k_in && v1[r] >= thr);
        as[r] = (a[r] >> 1) | ((uint64_t)((e_in && e0[r] >= thr) ? 1 : 0) << 63);
        bs[r] = (b[r] >> 1) | ((uint64_t)((e_in && e1[r] >= thr) ? 1 : 0) << 63);
    }
#pragma unroll
    for (int r = 0; r < kStrip; ++r) {
        const int32_t j = j0 + r;
        if (j >= d.ny) break;                       // (wave-uniform)
        const uint64_t all = a[r] & as[r] & a[r + 1] & as[r + 1] & b[r] & bs[r] & b[r + 1] & bs[r + 1];
        const uint64_t any = a[r] | as[r] | a[r + 1] | as[r + 1] | b[r] | bs[r] | b[r + 1] | bs[r + 1];
        const uint64_t active = any & ~all & cells;
        // the three lattice edges that start at the cell's corner 0: along x (needs j, k >= 1), y (k, i >= 1), z (i, j >= 1)
        const uint64_t qx = (j >= 1) ? ((a[r] ^ b[r]) & cells & k_ge1) : 0;
        const uint64_t qy = (i >= 1) ? ((a[r] ^ a[r + 1]) & cells & k_ge1) : 0;
        const uint64_t qz = (i >= 1 && j >= 1) ? ((a[r] ^ as[r]) & cells) : 0;
        if (lane == 0) {
            const int64_t ch = ((int64_t)i * d.ny + j) * d.cz + kc;
            masks[ch] = active;
            ranks[ch] = ((uint64_t)(__popcll(qx) + __popcll(qy) + __popcll(qz)) << 32) | (uint64_t)__popcll(active);
        }
    }
}

// What the scan's top level does with the grand total of the packed words: (vertices, triangles) unpacked, to the workspace and to the
// caller.  The packed halves never carry into each other (at most 2^30 vertices, 3 * 2^30 quads).
struct MeshTotalsTail {
    int64_t* totals_ws;
    int64_t* counts_dev;
    __device__ void operator()(uint64_t total) const {
        const int64_t v = (int64_t)(total & 0xffffffffull), t = 2 * (int64_t)(total >> 32);
        totals_ws[0] = v; totals_ws[1] = t;
        counts_dev[0] = v; counts_dev[1] = t;
    }
};

__device__ __forceinline__ int32_t rank_of(const uint64_t* __restrict__ masks, const uint64_t* __restrict__ ranks, const MeshDims& d, int32_t i, int32_t j, int32_t k) {
    const int64_t ch = ((int64_t)i * d.ny + j) * d.cz + (k >> 6);
    return (int32_t)(ranks[ch] & 0xffffffffull) + __popcll(masks[ch] & ((1ull << (k & 63)) - 1));
}

// The vertices and quads of one chunk, by one wave (all 64 lanes arrive; lanes along z).
__device__ __forceinline__ void write_chunk(const float* __restrict__ field, const MeshDims& d, float thr, const MeshBox& box, int64_t ch, uint64_t active,
                                            const uint64_t* __restrict__ masks, const uint64_t* __restrict__ ranks, float* __restrict__ vertices,
                                            int64_t vertex_capacity, int32_t* __restrict__ faces, int64_t face_capacity) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t kc = (int32_t)(ch % d.cz);
    const int32_t j = (int32_t)((ch / d.cz) % d.ny);
    const int32_t i = (int32_t)(ch / ((int64_t)d.cz * d.ny));
    const int32_t k = kc * 64 + lane;
    const uint64_t packed = ranks[ch];
    const uint64_t below = (1ull << lane) - 1;
    const bool mine = (active >> lane) & 1;
    bool qx = false, qy = false, qz = false, in0 = false;
    if (mine) {                                      // (k < nz: the count pass masked the cells past the row's end)
        const int64_t row_stride = (int64_t)d.nz + 1;
        const float* c0 = field + ((int64_t)i * (d.ny + 1) + j) * row_stride + k;
        const float* c1 = c0 + (int64_t)(d.ny + 1) * row_stride;
        float v[8];                                  // corner 4 dx + 2 dy + dz
        v[0] = c0[0]; v[1] = c0[1]; v[2] = c0[row_stride]; v[3] = c0[row_stride + 1];
        v[4] = c1[0]; v[5] = c1[1]; v[6] = c1[row_stride]; v[7] = c1[row_stride + 1];
        bool in[8];
        float w[3];
        mesh_cell_vertex(v, thr, i, j, k, box, in, w);          // (mesh_device.hpp: the arithmetic the brick unit shares)
        const int64_t rank = (int64_t)(packed & 0xffffffffull) + __popcll(active & below);
        if (rank < vertex_capacity) {
            vertices[3 * rank + 0] = w[0];
            vertices[3 * rank + 1] = w[1];
            vertices[3 * rank + 2] = w[2];
        }
        in0 = in[0];
        qx = (in[0] != in[4]) && j >= 1 && k >= 1;
        qy = (in[0] != in[2]) && k >= 1 && i >= 1;
        qz = (in[0] != in[1]) && i >= 1 && j >= 1;
    }
    const uint64_t mx = __ballot(qx), my = __ballot(qy), mz = __ballot(qz);
    int64_t quad = (int64_t)(packed >> 32) + __popcll(mx & below) + __popcll(my & below) + __popcll(mz & below);
    const int32_t p[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool emit = a == 0 ? qx : (a == 1 ? qy : qz);
        if (!emit) continue;
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        int32_t cell[3] = {p[0], p[1], p[2]};
        int32_t q[4];
        q[2] = rank_of(masks, ranks, d, cell[0], cell[1], cell[2]);            // p
        cell[b] -= 1;
        q[3] = rank_of(masks, ranks, d, cell[0], cell[1], cell[2]);            // p - e_b
        cell[c] -= 1;
        q[0] = rank_of(masks, ranks, d, cell[0], cell[1], cell[2]);            // p - e_b - e_c
        cell[b] += 1;
        q[1] = rank_of(masks, ranks, d, cell[0], cell[1], cell[2]);            // p - e_c
        if (!in0) { const int32_t t0 = q[0], t1 = q[1]; q[0] = q[3]; q[1] = q[2]; q[2] = t1; q[3] = t0; }
        const int64_t tri = 2 * quad;
        if (tri + 1 < face_capacity) {
            int32_t* f = faces + 3 * tri;
            f[0] = q[0]; f[1] = q[1]; f[2] = q[2];
            f[3] = q[0]; f[4] = q[2]; f[5] = q[3];
        }
        ++quad;
    }
}

// A wave takes 64 consecutive chunks: their masks are one coalesced load, and only the chunks with an active cell are visited (a chunk
// without one has neither a vertex nor a quad: an edge with differing ends makes its four cells active).
__global__ void __launch_bounds__(256) mesh_write_kernel(const float* __restrict__ field, MeshDims d, float thr, MeshBox box, int64_t n_chunks,
                                                         const uint64_t* __restrict__ masks, const uint64_t* __restrict__ ranks, float* __restrict__ vertices,
                                                         int64_t vertex_capacity, int32_t* __restrict__ faces, int64_t face_capacity) {
    const int64_t first = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 64;
    if (first >= n_chunks) return;                  // (wave-uniform)
    const int32_t lane = threadIdx.x & 63;
    const uint64_t own = first + lane < n_chunks ? masks[first + lane] : 0;
    uint64_t todo = __ballot(own != 0);
    while (todo) {                                  // (wave-uniform)
        const int c = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t active = (uint64_t)__shfl((unsigned long long)own, c);
        write_chunk(field, d, thr, box, first + c, active, masks, ranks, vertices, vertex_capacity, faces, face_capacity);
    }
}

static int mesh_dims_check(const char* who, int32_t nx, int32_t ny, int32_t nz) {
    PERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "%s: a lattice of %d x %d x %d cells has a dimension below 1", who, (int)nx, (int)ny, (int)nz);
    PERF_REQUIRE((int64_t)nx * ny <= PERF_MESH_MAX_CELLS && (int64_t)nx * ny * nz <= PERF_MESH_MAX_CELLS,
                 "%s: %d x %d x %d cells are more than 2^30 (vertex indices are int32)", who, (int)nx, (int)ny, (int)nz);
    return PERF_OK;
}

static int mesh_workspace_check(const char* who, int32_t nx, int32_t ny, int32_t nz, const void* workspace, int64_t workspace_bytes) {
    return workspace_check(who, perf_mesh_workspace_bytes(nx, ny, nz), workspace, workspace_bytes);
}

}  // namespace perf

using namespace perf;

extern "C" int perf_mesh_version(void) { return PERF_MESH_ABI_VERSION; }

extern "C" int64_t perf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (mesh_dims_check("perf_mesh_workspace_bytes", nx, ny, nz) != PERF_OK) return -1;
    const int64_t chunks = chunks_of(nx, ny, nz);
    return ((2 * chunks + scan_words(chunks) + 2 + 1) & ~(int64_t)1) * (int64_t)sizeof(uint64_t);      // (a multiple of 16)
}

extern "C" int perf_mesh_count(const float* field, int32_t nx, int32_t ny, int32_t nz, float thr, void* workspace, int64_t workspace_bytes,
                               int64_t* counts_dev, void* stream) {
    PERF_REQUIRE(field, "perf_mesh_count: NULL input (field)");
    PERF_REQUIRE(counts_dev, "perf_mesh_count: NULL output (counts_dev)");
    if (int rc = mesh_dims_check("perf_mesh_count", nx, ny, nz)) return rc;
    PERF_REQUIRE(thr - thr == 0.0f, "perf_mesh_count: the threshold is not finite");
    if (int rc = mesh_workspace_check("perf_mesh_count", nx, ny, nz, workspace, workspace_bytes)) return rc;
    MeshDims d{nx, ny, nz, (int32_t)div_up(nz, 64)};
    const int64_t chunks = chunks_of(nx, ny, nz);
    uint64_t* masks = (uint64_t*)workspace;
    uint64_t* ranks = masks + chunks;
    uint64_t* level = ranks + chunks;
    int64_t* totals = (int64_t*)(level + scan_words(chunks));
    const int64_t n_strips = (int64_t)nx * div_up(ny, kStrip) * d.cz;
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)div_up(n_strips, 4)), dim3(256), 0, as_stream(stream), field, d, thr, n_strips, masks, ranks);
    scan_u64(ranks, chunks, level, as_stream(stream), MeshTotalsTail{totals, counts_dev});
    PERF_LAUNCH_CHECK("perf_mesh_count");
    return PERF_OK;
}

extern "C" int perf_mesh_write(const float* field, int32_t nx, int32_t ny, int32_t nz, float thr, const float* lo, const float* hi,
                               const void* workspace, int64_t workspace_bytes, float* vertices, int64_t vertex_capacity, int32_t* faces,
                               int64_t face_capacity, void* stream) {
    PERF_REQUIRE(field && lo && hi, "perf_mesh_write: NULL input (field, lo or hi)");
    PERF_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, "perf_mesh_write: negative capacity");
    PERF_REQUIRE((vertices || vertex_capacity == 0) && (faces || face_capacity == 0), "perf_mesh_write: NULL output with a capacity above 0");
    if (int rc = mesh_dims_check("perf_mesh_write", nx, ny, nz)) return rc;
    PERF_REQUIRE(thr - thr == 0.0f, "perf_mesh_write: the threshold is not finite");
    for (int a = 0; a < 3; ++a)
        PERF_REQUIRE(hi[a] > lo[a] && hi[a] - hi[a] == 0.0f && lo[a] - lo[a] == 0.0f, "perf_mesh_write: the box needs finite hi > lo on every axis (axis %d: lo %g, hi %g)", a, (double)lo[a],
                     (double)hi[a]);
    if (int rc = mesh_workspace_check("perf_mesh_write", nx, ny, nz, workspace, workspace_bytes)) return rc;
    MeshDims d{nx, ny, nz, (int32_t)div_up(nz, 64)};
    const int64_t chunks = chunks_of(nx, ny, nz);
    const uint64_t* masks = (const uint64_t*)workspace;
    const uint64_t* ranks = masks + chunks;
    const int64_t* totals_dev = (const int64_t*)(ranks + chunks + scan_words(chunks));
    int64_t totals[2] = {0, 0};
    if (hipMemcpyAsync(totals, totals_dev, sizeof(totals), hipMemcpyDeviceToHost, as_stream(stream)) != hipSuccess ||
        hipStreamSynchronize(as_stream(stream)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("perf_mesh_write: reading the counted totals back failed");
        return PERF_E_LAUNCH;
    }
    PERF_REQUIRE(vertex_capacity >= totals[0], "perf_mesh_write: room for %lld vertices, %lld were counted", (long long)vertex_capacity, (long long)totals[0]);
    PERF_REQUIRE(face_capacity >= totals[1], "perf_mesh_write: room for %lld faces, %lld were counted", (long long)face_capacity, (long long)totals[1]);
    if (totals[0] == 0) return PERF_OK;              // (no active cell: no quad either)
    MeshBox box;
    const int32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = (double)lo[a];
        box.scale[a] = ((double)hi[a] - (double)lo[a]) / (double)n[a];
    }
    hipLaunchKernelGGL(mesh_write_kernel, dim3((unsigned)div_up(chunks, 256)), dim3(256), 0, as_stream(stream), field, d, thr, box, chunks, masks, ranks, vertices,
                       vertex_capacity, faces, face_capacity);
    PERF_LAUNCH_CHECK("perf_mesh_write");
    return PERF_OK;
}
