/* A triangle mesh of a scalar lattice by naive surface nets, on the device: a sixth header of libperf_hip.so, versioned on its own --
 * PERF_MESH_ABI_VERSION / perf_mesh_version(), recorded in include/perf_hip_mesh.abi.json (`python tools/abi_digest.py --mesh [--write]`).
 * Error codes and conventions are those of perf_hip.h: raw device pointers, counts and a stream; an integer return code, the reason of a
 * refusal in perf_last_error(); a caller-owned workspace sized by perf_mesh_workspace_bytes; nothing is allocated; everything that is
 * refused is refused before anything is launched.  No case tables and no atomics: the order of vertices and faces comes from a scan, so
 * two runs on one field give identical bits.
 *
 * The algorithm (restated in float64 numpy by tests/mesh_reference.py):
 *   field: fp32 [nx+1, ny+1, nz+1] corner values in C order, z fastest.  A corner is inside iff field >= thr (a NaN is outside).
 *   Vertices.  Cell (i, j, k), 0 <= i < nx etc., is active iff its eight corners are not all alike; it owns one vertex.  In lattice
 *     units the vertex is (i, j, k) + the mean of the crossing points on those of its 12 edges whose ends differ; edges are the pairs
 *     a < b of corner offsets in {0,1}^3 (corner number 4 dx + 2 dy + dz) in lexicographic order of (a, b); on an edge from value va to
 *     vb the crossing is at t = clamp((thr - va) / (vb - va), 0, 1), a NaN t (infinite corners) replaced by 1/2.  In world units the
 *     vertex is lo + p (hi - lo) / n per axis.  A vertex's index is the rank of its cell among the active cells in linear cell order
 *     ((i ny + j) nz + k).
 *   Faces.  A lattice edge from corner p along axis a (p[a] < n[a]) whose ends differ emits one quad iff, with b = (a+1)%3 and
 *     c = (a+2)%3, 1 <= p[b] <= n[b]-1 and 1 <= p[c] <= n[c]-1 (all four cells around it exist): the vertices of the cells p-e_b-e_c,
 *     p-e_c, p, p-e_b, in this order if p is inside and reversed otherwise, split as (q0,q1,q2), (q0,q2,q3).  Faces are ordered by
 *     (linear corner index of p) * 3 + a, an edge's two triangles adjacent.  Normals then point from high values to low.
 *   Arithmetic.  A vertex is carried in double between the fp32 corner loads and its fp32 store: ONE fp32 rounding per coordinate.
 *
 * Protocol: count -> the caller reads the two totals (the one host synchronisation it needs) and allocates -> write.
 *
 * Workspace, in 8-byte words, with C = nx ny ceil(nz / 64) chunks of 64 cells along z: C words of the chunks' active masks (the per-cell
 * code is this one bit), C words of the chunks' ranks -- (quads before the chunk) << 32 | (vertices before it) --, the scan's partial
 * sums (C/256 + C/256^2 + ... words) and the two totals.  That is 0.25 bytes per cell where nz is a multiple of 64 and at most 16.1
 * bytes per cell (nz == 1); the field itself takes 4 bytes per corner, 4.3 GB at the documented ceiling of 1024^3 cells (2^30 cells:
 * vertex indices are int32). */
#ifndef PERF_HIP_MESH_H
#define PERF_HIP_MESH_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESH_ABI_VERSION 1
#define PERF_MESH_MAX_CELLS 1073741824 /* 2^30 */

int perf_mesh_version(void);            /* == PERF_MESH_ABI_VERSION of the header the library was built from */

/* Bytes of the workspace of one lattice (a multiple of 16); -1 with a reason: a dimension < 1 or more than PERF_MESH_MAX_CELLS cells. */
int64_t perf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);

/* perf_mesh_count: classifies every cell (one streaming read of the field), leaves the chunks' masks and ranks in the workspace and
 * counts_dev [2] = (vertices, triangles) on the device.  workspace: 16-byte aligned, >= perf_mesh_workspace_bytes(nx, ny, nz).
 * thr must be finite. */
int perf_mesh_count(const float* field, int32_t nx, int32_t ny, int32_t nz, float thr, void* workspace, int64_t workspace_bytes,
                    int64_t* counts_dev, void* stream);

/* perf_mesh_write: vertices [V, 3] fp32 and faces [F, 3] int32 of the SAME field, thr and workspace perf_mesh_count was given (the
 * stream's order puts it after the count).  lo, hi: HOST pointers to the box's three lower and upper bounds, hi > lo on every axis.
 * vertex_capacity / face_capacity: rows the two arrays hold; capacities below the counted totals are refused: the call reads the two
 * totals back from the workspace (16 bytes, after the stream has drained -- right after the caller's own read this costs no wait), so
 * it is not for stream capture.  vertices / faces may be NULL when their capacity is 0. */
int perf_mesh_write(const float* field, int32_t nx, int32_t ny, int32_t nz, float thr, const float* lo, const float* hi,
                    const void* workspace, int64_t workspace_bytes, float* vertices, int64_t vertex_capacity, int32_t* faces,
                    int64_t face_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESH_H */
