/* The closest point of a triangle mesh to each of a batch of query points, on the uniform grid of perf_hip_meshray.h: a STAGED header of
 * libperf_hip.so (include/staged/: bound and version-checked like every unit, not yet in the pinned table), versioned on its own --
 * PERF_MESHNEAR_ABI_VERSION / perf_meshnear_version(), recorded in include/staged/perf_hip_meshnear.abi.json
 * (`python tools/abi_digest.py --meshnear [--write]`).  Error codes and conventions are those of perf_hip.h: raw device pointers, 64-bit
 * counts and a stream; an integer return code, the reason of a refusal in perf_last_error(); the memory is the caller's, nothing is
 * allocated; everything that is refused is refused before anything is launched.
 *
 * The statement.
 *   The rule, per face.  A point p and a face (a, b, c); every value is a DOUBLE formed from the fp32 inputs, each operation rounds once,
 *     nothing is contracted; x . y = (xx yx + xy yy) + xz yz:
 *       ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
 *       d1 = ab . ap, d2 = ac . ap, d3 = ab . bp, d4 = ac . bp, d5 = ab . cp, d6 = ac . cp
 *       vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e = d4 - d3, g = d5 - d6
 *     the FIRST of these tests that holds decides the region (every comparison false on NaN):
 *       0  p equals a vertex:  ap == 0: as 1;  else bp == 0: as 2;  else cp == 0: as 3
 *       1  vertex a:  d1 <= 0 and d2 <= 0                                          u = 0, v = 0, r = ap
 *       2  vertex b:  d3 >= 0 and d4 <= d3                                         u = 1, v = 0, r = bp
 *       3  vertex c:  d6 >= 0 and d5 <= d6                                         u = 0, v = 1, r = cp
 *       4  edge ab:   vc <= 0 and d1 >= 0 and d3 <= 0 and (d1 - d3) > 0            u = d1 / (d1 - d3), v = 0
 *       5  edge ac:   vb <= 0 and d2 >= 0 and d6 <= 0 and (d2 - d6) > 0            u = 0, v = d2 / (d2 - d6)
 *       6  edge bc:   va <= 0 and e >= 0 and g >= 0 and (e + g) > 0                v = e / (e + g), u = 1 - v
 *       7  interior:  va > 0 and vb > 0 and vc > 0                                 den = (va + vb) + vc, u = vb / den, v = vc / den
 *       8  otherwise (a face that rounding has flattened): the vertex with the smallest |r|^2 of ap, bp, cp, the first of equals, as 1 - 3
 *     in the regions 4 - 7:  q = (a + u ab) + v ac, r = p - q;  in every region  dist2 = (rx rx + ry ry) + rz rz.
 *     Every division's denominator is tested first (> 0).  Test 0 is there because b - a need not be exact in double: with it a point equal
 *     to a vertex of the face lands in that vertex's region with dist2 == 0 exactly, whatever the other vertices are.  A degenerate face
 *     (collinear or coincident vertices) is answered by its vertex and edge regions: its va, vb, vc are not all positive.  Every answer
 *     is a point of the face: a vertex, a point of an edge with its parameter in [0, 1], or u, v > 0 and u + v < 1 up to one rounding.
 *     A face with an index outside [0, V) or with a vertex that is not finite is never the answer.  No square root is taken: dist2
 *     leaves as a double, and no result rests on the rounding of the device's sqrt.
 *   The answer, perf_meshnear_query: the lexicographic minimum of (dist2, face index) over ALL faces, never "over the cells visited".
 *     dist2_out float64 [N], face_out int32 [N], u_out = (float)u and v_out = (float)v where they are asked for: the closest point is
 *     (1 - u - v) a + u b + v c.  A point that is NaN or infinite writes +inf, -1, 0, 0 and reads nothing; the same is written when there
 *     is no valid face, and when the minimum's dist2 exceeds (double)max_distance * (double)max_distance (max_distance +inf: no limit).
 *   The grid is the one perf_meshray_grid_count / perf_meshray_grid_write of perf_hip_meshray.h make (this header includes nothing and
 *     restates what it reads): origin [3] fp32, cell fp32 (> 0, finite), dims [3] int32 (each >= 1) with a product within
 *     PERF_MESHNEAR_MAX_CELLS; cell (i, j, k) at (i ny + j) nz + k; cell c lists refs[cell_offsets[c] .. cell_offsets[c + 1]) (the last
 *     cell up to n_refs); the margin is m = cell / 8: a face is listed in every cell whose index range, per axis, overlaps
 *     [floor((min - m - origin) / cell), floor((max + m - origin) / cell)], clamped to the grid; a face wholly outside the box is listed
 *     nowhere.
 *   The search.  It starts at the cell that holds the point, floor((p - origin) / cell) in double, clamped to the grid for a point outside
 *     the box, and visits the cells in shells of growing Chebyshev radius r = 0, 1, ...; every listed face of a new cell is tested by the
 *     rule above (a face listed in several cells may be tested more than once; the minimum does not care).  After shell r the visited
 *     block is an axis-aligned box of cells.  D is the smallest distance, along its own axis, from the point to a side of that block that
 *     is not the grid's own boundary (nothing is listed beyond the grid's boundary); a negative D counts as 0.  The search stops as soon
 *     as best dist2 <= D * D, or D > max_distance, or the block is the whole grid: at most max(nx, ny, nz) shells.
 *     Why this is exact: a face not yet visited is listed in no cell of the block, so its bounding box widened by m misses the block along
 *     some axis, beyond a side that is not the grid's boundary; every point of it is at least D + m from the point.  The rule answers a
 *     point of the face, and its rounding error and that of D are many orders below m; so the face's computed dist2 exceeds D * D: it can
 *     neither win nor tie (and with D > max_distance it lies beyond the limit).  The result is the brute-force one whenever the box holds
 *     the faces' vertices, and does not depend on cell or dims.  No atomics, one plain store per output: bit-identical from run to run.
 *   The cost.  A point at distance d from the mesh visits the O((d / cell)^3) cells around it, empty or not: a point far from the mesh, or
 *     far outside a fine grid, is slow.  max_distance is the way to bound it: the search ends once D exceeds it.
 *   What it does NOT do: no BVH; no sparse or two-level grid; no empty-space skipping; no signed distance; no square root; no exact
 *     (unsampled) Hausdorff distance -- the deviation of perf_amd/mesh.py is a sampled one.
 *   Refusals.  NULL inputs or outputs where the count is positive (u_out and v_out may be NULL), a NULL origin or dims; cell <= 0 or not
 *     finite, an origin that is not finite; a dim below 1; more cells than PERF_MESHNEAR_MAX_CELLS; negative counts; V above
 *     PERF_MESHNEAR_MAX_VERTICES (2^30), F above PERF_MESHNEAR_MAX_FACES (2^31 - 1); n_refs negative or >= 2^31; more than 2^38 points;
 *     max_distance NaN or negative. */
#ifndef PERF_HIP_MESHNEAR_H
#define PERF_HIP_MESHNEAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHNEAR_ABI_VERSION 1
#define PERF_MESHNEAR_MAX_CELLS 16777216       /* 2^24: PERF_MESHRAY_MAX_CELLS, restated */
#define PERF_MESHNEAR_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHNEAR_MAX_FACES 2147483647    /* 2^31 - 1 */

int perf_meshnear_version(void); /* == PERF_MESHNEAR_ABI_VERSION of the header the library was built from */

/* vertices: device fp32 [n_vertices, 3]; faces: device int32 [n_faces, 3]; origin: HOST fp32 [3]; dims: HOST int32 [3]; cell_offsets:
 * device int32 [dims[0] * dims[1] * dims[2]]; refs: device int32 [n_refs]; points: device fp32 [n_points, 3]; dist2_out: device float64
 * [n_points]; face_out: device int32 [n_points]; u_out, v_out: device fp32 [n_points] or NULL.  vertices may be NULL when n_vertices is
 * 0, faces when n_faces is 0, refs when n_refs is 0. */
int perf_meshnear_query(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell,
                        const int32_t* dims, const int32_t* cell_offsets, const int32_t* refs, int64_t n_refs, const float* points,
                        int64_t n_points, float max_distance, double* dist2_out, int32_t* face_out, float* u_out, float* v_out,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHNEAR_H */
