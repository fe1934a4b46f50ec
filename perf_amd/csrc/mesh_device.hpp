// The vertex of one active surface-nets cell (include/perf_hip_mesh.h): shared by the dense unit (mesh.hip) and the brick unit
// (brickmesh.hip), so that both store the same bits for the same eight corner values, cell and box.
#pragma once
#include "common.hpp"

namespace perf {

struct MeshBox {
    double lo[3], scale[3];          // world = lo + p * scale, scale = (hi - lo) / n
};

// v: the cell's corner values, corner 4 dx + 2 dy + dz; (i, j, k): the cell in the whole lattice.  -> in[c] = v[c] >= thr and the world
// position, carried in double and rounded to fp32 ONCE.  The cell must be active (some in[] differ): crossings > 0.
__device__ __forceinline__ void mesh_cell_vertex(const float (&v)[8], float thr, int32_t i, int32_t j, int32_t k, const MeshBox& box, bool (&in)[8], float (&out)[3]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = v[c] >= thr;
    // the 12 edges: pairs a < b of corners that differ in one offset, in lexicographic order of (a, b)
    constexpr int ea[12] = {0, 0, 0, 1, 1, 2, 2, 3, 4, 4, 5, 6};
    constexpr int eb[12] = {1, 2, 4, 3, 5, 3, 6, 7, 5, 6, 7, 7};
    double sum[3] = {0.0, 0.0, 0.0};
    int crossings = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int a = ea[e], b = eb[e];
        if (in[a] != in[b]) {
            double t = ((double)thr - (double)v[a]) / ((double)v[b] - (double)v[a]);
            if (t != t) t = 0.5;
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            const int axis = (b - a) == 4 ? 0 : ((b - a) == 2 ? 1 : 2);
            sum[0] += (axis == 0) ? t : (double)((a >> 2) & 1);
            sum[1] += (axis == 1) ? t : (double)((a >> 1) & 1);
            sum[2] += (axis == 2) ? t : (double)(a & 1);
            ++crossings;
        }
    }
    const double px = (double)i + sum[0] / (double)crossings, py = (double)j + sum[1] / (double)crossings, pz = (double)k + sum[2] / (double)crossings;
    out[0] = (float)(box.lo[0] + px * box.scale[0]);
    out[1] = (float)(box.lo[1] + py * box.scale[1]);
    out[2] = (float)(box.lo[2] + pz * box.scale[2]);
}

}  // namespace perf
