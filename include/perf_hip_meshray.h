/* Rays against a triangle mesh on a uniform grid: closest hit, any hit, and the occlusion of the segments from a mesh's vertices to the
 * views' centres: a twelfth header of libperf_hip.so, versioned on its own -- PERF_MESHRAY_ABI_VERSION / perf_meshray_version(),
 * recorded in include/perf_hip_meshray.abi.json (`python tools/abi_digest.py --meshray [--write]`).  Error codes and conventions are
 * those of perf_hip.h: raw device pointers, 64-bit counts and a stream; an integer return code, the reason of a refusal in
 * perf_last_error(); the memory is the caller's, nothing is allocated; everything that is refused is refused before anything is launched.
 *
 * The statement.
 *   The rule, per face.  A ray (o, d) and a face (a, b, c); every value is a DOUBLE formed from the fp32 inputs, each operation rounds
 *     once, nothing is contracted:
 *       e1 = b - a, e2 = c - a
 *       p  = (dy e2z - dz e2y,  dz e2x - dx e2z,  dx e2y - dy e2x)
 *       det = (e1x px + e1y py) + e1z pz              det == 0 or NaN: no hit
 *       s  = o - a
 *       u  = ((sx px + sy py) + sz pz) / det
 *       q  = (sy e1z - sz e1y,  sz e1x - sx e1z,  sx e1y - sy e1x)
 *       v  = ((dx qx + dy qy) + dz qz) / det
 *       t  = ((e2x qx + e2y qy) + e2z qz) / det
 *       hit  <=>  u >= 0 and v >= 0 and (u + v) <= 1 and t_min <= t <= t_max      (every comparison false on NaN)
 *     The test is two-sided: no backface culling.  The rule is PER FACE and therefore NOT WATERTIGHT along shared edges: rounding can
 *     put a ray that runs through an edge outside both of its faces (on the symmetric hollow sphere of the tests, seen from the centre
 *     of its box, one segment in 1,100 slips through).  A face with an index outside [0, V) or with a vertex that is not finite can
 *     never be hit.
 *   Closest hit, perf_meshray_cast with any_hit == 0: the lexicographic minimum of (t, face index) over ALL faces that hit, never "over
 *     the cells visited".  t_out = (float)t, face_out the index as int32, u_out = (float)u and v_out = (float)v where they are asked
 *     for; a ray with no hit writes +inf, -1, 0, 0.
 *   Any hit, any_hit == 1: hit_out uint8, 1 iff some face hits; nothing else is written.
 *   Segment occlusion, perf_meshray_occluded: vertex v at p and view k with centre c_k: the ray o = p, d = c_k - p (formed in double); a
 *     hit requires the STRICT 0 < t < 1; faces that name index v are not tested for v's segments (exact: no epsilon); the test is
 *     evaluated only where bit k of mask_bits[v] is set.  occluded_bits int64 [V] is a subset of the mask; bits >= K are 0; K <= 64.
 *   The grid.  The box is the caller's: origin [3] fp32, cell fp32 (> 0, finite), dims [3] int32 (each >= 1) with a product within
 *     PERF_MESHRAY_MAX_CELLS (2^24: 64 MiB of int32 counts and 64 MiB of int32 offsets).  The margin is m = cell / 8.  A face is listed
 *     in every cell whose index range, per axis, overlaps
 *       [floor((min - m - origin) / cell), floor((max + m - origin) / cell)]
 *     in double, ((min - m) - origin) / cell, clamped to the grid; a face wholly outside the box is listed nowhere, and so is a face
 *     that can never be hit: the smallest index of such a face is left in bad_face_dev (-1: none; one integer atomicMin per such face).
 *     The protocol is count -> scan -> write: perf_meshray_grid_count fills the per-cell int32 counts with integer atomicAdd only; the
 *     caller scans them exclusively into int32 offsets (perf_exclusive_scan_i32) and reads the total R back, the one host read;
 *     perf_meshray_grid_write fills refs int32 [R] and leaves the counts 0.  The order of the references inside a cell is unspecified
 *     and no result depends on it.  R >= 2^31 is refused.  Both passes run one thread per face over the cells of its range: a face as
 *     large as the box costs one lane as many atomics as the grid has cells, 2^24 at the most -- bounded, and slow only for such a face.
 *   The walk.  The ray is clipped to the box widened by m, in double; the cells are walked by a 3-D DDA in double, at most
 *     nx + ny + nz + 2 steps; every listed face of a cell is tested by the rule above.  Closest hit stops once the entry parameter of the
 *     next cell exceeds the best t, any hit at the first hit.  The grid only skips faces that cannot hit: a hit point lies in its face's
 *     bounding box, the walk's rounding error is many orders below m, so a visited cell lists the face, and the result is the brute-force
 *     one whenever the box holds the faces' vertices (a hit point outside the caller's box widened by m is not found).  d = 0, a NaN or
 *     an infinite ray, a ray that misses the box: no hit, nothing is read.  No floating-point atomics, no atomics at all in the walk, one
 *     plain store per output: the results are bit-identical from run to run and do not depend on cell or dims.
 *   What it does NOT do: no BVH; no sparse or two-level grid (the cell array is dense); no texture bake; no occlusion in the colouring of
 *     perf_hip_meshcolor.h (its blend would need a new ABI version of that header); no watertightness along shared edges.
 *   Refusals.  NULL inputs or outputs where the count is positive, a NULL origin, dims or bad_face_dev; cell <= 0 or not finite, an
 *     origin that is not finite; a dim below 1; more cells than PERF_MESHRAY_MAX_CELLS; K outside 0 .. 64; negative counts; V above
 *     PERF_MESHRAY_MAX_VERTICES (2^30), F above PERF_MESHRAY_MAX_FACES (2^31 - 1); a capacity of refs below the counted R, R negative or
 *     >= 2^31; t_min or t_max NaN; any_hit other than 0 or 1. */
#ifndef PERF_HIP_MESHRAY_H
#define PERF_HIP_MESHRAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHRAY_ABI_VERSION 1
#define PERF_MESHRAY_MAX_CELLS 16777216       /* 2^24 */
#define PERF_MESHRAY_MAX_VIEWS 64
#define PERF_MESHRAY_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHRAY_MAX_FACES 2147483647    /* 2^31 - 1 */

int perf_meshray_version(void); /* == PERF_MESHRAY_ABI_VERSION of the header the library was built from */

/* The counts.  vertices: device fp32 [n_vertices, 3]; faces: device int32 [n_faces, 3]; origin: HOST fp32 [3]; dims: HOST int32 [3];
 * cell_counts: device int32 [dims[0] * dims[1] * dims[2]], zeroed by the call, cell (i, j, k) at (i ny + j) nz + k; bad_face_dev: device
 * int64 [1].  vertices may be NULL when n_vertices is 0, faces when n_faces is 0. */
int perf_meshray_grid_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin,
                            float cell, const int32_t* dims, int32_t* cell_counts, int64_t* bad_face_dev, void* stream);

/* The references.  cell_counts: what perf_meshray_grid_count left, consumed (left 0) by the call; cell_offsets: their exclusive scan;
 * n_refs_counted: the scan's total R as the caller read it; refs: device int32 [ref_capacity], ref_capacity >= R.  No reference is
 * written at or beyond ref_capacity whatever the counts hold.  refs may be NULL when R is 0. */
int perf_meshray_grid_write(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin,
                            float cell, const int32_t* dims, int32_t* cell_counts, const int32_t* cell_offsets, int64_t n_refs_counted,
                            int32_t* refs, int64_t ref_capacity, void* stream);

/* Closest hit (any_hit 0: t_out fp32 [n_rays], face_out int32 [n_rays], u_out and v_out fp32 [n_rays] or NULL) or any hit (any_hit 1:
 * hit_out uint8 [n_rays]) of rays_o, rays_d fp32 [n_rays, 3] against the mesh the grid (cell_offsets, refs [n_refs]) was built of. */
int perf_meshray_cast(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin, float cell,
                      const int32_t* dims, const int32_t* cell_offsets, const int32_t* refs, int64_t n_refs, const float* rays_o,
                      const float* rays_d, int64_t n_rays, float t_min, float t_max, int32_t any_hit, float* t_out, int32_t* face_out,
                      float* u_out, float* v_out, uint8_t* hit_out, void* stream);

/* Segment occlusion.  centres: device fp32 [n_views, 3]; mask_bits, occluded_bits: device int64 [n_vertices]. */
int perf_meshray_occluded(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* origin,
                          float cell, const int32_t* dims, const int32_t* cell_offsets, const int32_t* refs, int64_t n_refs,
                          const float* centres, int32_t n_views, const int64_t* mask_bits, int64_t* occluded_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHRAY_H */
