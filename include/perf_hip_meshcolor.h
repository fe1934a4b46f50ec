/* Colour the vertices of a triangle mesh from the registered panoramas, and build geometric vertex normals from its faces: an eleventh
 * header of libperf_hip.so, versioned on its own -- PERF_MESHCOLOR_ABI_VERSION / perf_meshcolor_version(), recorded in
 * include/perf_hip_meshcolor.abi.json (`python tools/abi_digest.py --meshcolor [--write]`).  Error codes and conventions are those of
 * perf_hip.h: raw device pointers, counts and a stream; an integer return code, the reason of a refusal in perf_last_error(); nothing is
 * allocated and there is no workspace; everything that is refused is refused before anything is launched.  The views are the
 * perf_meshvis_view array of perf_hip_meshvis.h, unchanged.
 *
 * The statement.
 *   Stage A, perf_meshcolor_normal_sums then perf_meshcolor_normals: vertex normals from faces.  For a face (a, b, c) with all indices
 *     in [0, V) the area-weighted normal is formed in DOUBLE from the fp32 vertices, one rounding per operation, nothing contracted, as
 *     stage 2 of the cull writes it:
 *       e1 = b - a, e2 = c - a                                        (per component)
 *       n  = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)
 *       q_c = llrint(n_c * 2^s)                                       (s = scale_log2, round to nearest even; the product is exact)
 *     If any n_c * 2^s is not finite or has magnitude >= 2^62 the face contributes nothing (a NaN or an infinite vertex).  Otherwise
 *     the three q_c are added to acc[a], acc[b] and acc[c] (int64 [V, 3], zeroed by the call) with 64-bit integer atomicAdd: there are
 *     no floating-point atomics, so the sums do not depend on the faces' order and are bit-identical from run to run.  Sums wrap modulo
 *     2^64 as int64 does: with terms below 2^62 two faces at one vertex can already wrap; with the scale the Python side chooses,
 *     s = 40 - ceil(log2(D^2)) for a box of squared diagonal D^2 (|e1 x e2| <= D^2: every term is below 2^40), a vertex needs a valence
 *     of 2^23 faces.  A face with an index outside [0, V) is not followed; the smallest index of such a face is left in bad_face_dev
 *     (-1: none; one integer atomicMin per such face).
 *     The second call forms the unit normal in double:
 *       A = (double)acc,  len = sqrt((Ax Ax + Ay Ay) + Az Az),  normal_c = (float)(A_c / len),  and exactly 0 where len == 0
 *     (a vertex no face names, a vertex whose faces cancel).
 *   Stage B, perf_meshcolor_blend: the colours.  vertices fp32 [V, 3], normals fp32 [V, 3], K <= 64 views and K colour maps, each fp32
 *     [H, W, 3] OF THE VIEW'S OWN DISTANCE MAP'S HEIGHT AND WIDTH -> colors fp32 [V, 3], weight fp32 [V], used_bits int64 [V], best_view
 *     int8 [V].  One thread per vertex; the views and the map pointers are staged in LDS with the workgroup's 256 vertices; the loop
 *     over k ascends.  For view k:
 *     1. dist, the four tap addresses with their bounds tests, the four weights and proj are THE LOOK-UP OF perf_meshvis_vertex_bits
 *        RESTATED LINE FOR LINE (fp32, one rounding per operation, asinf / atan2f, align_corners=False, the border clamp).  The colour
 *        sample c_k is the same four-tap accumulation per channel over the colour map: fp32, in nw / ne / sw / se order, with the same
 *        weights and the same border clamp.  There is no wrap at the seam: the half pixel at the +-pi column is clamped, which is the
 *        reference's own grid_sample behaviour.
 *     2. The view is visible iff dist < proj + tol: bit for bit the `visible` word of perf_meshvis_vertex_bits (a pixel the panorama
 *        did not store has proj = 0).  The view is additionally skipped unless dist > 0 and dist is finite.
 *     3. With facing, in double from the fp32 values, nothing contracted: g = t_k - p, s = (Nx gx + Ny gy) + Nz gz; the view is
 *        skipped unless s > 0 (exact from the fp32 inputs, as the cull's facing test);
 *          cos = s / (sqrt((Nx Nx + Ny Ny) + Nz Nz) * sqrt((gx gx + gy gy) + gz gz)).
 *     4. w_k = cos^power / ((double)dist * (double)dist) with facing (cos^power by power - 1 successive multiplications), and
 *        1 / ((double)dist * (double)dist) without: a panorama pixel's footprint on the surface grows as dist^2 / cos.  A view whose
 *        w_k is not > 0 (an underflow, a NaN from infinite normals) is skipped.  w_k is finite in double (dist >= 2^-75); the fp32
 *        weight below overflows to infinity only for a vertex within 2^-64 of a view's centre.
 *     5. A view that passes sets bit k of used_bits.  select 0, blend: num += w_k * (double)c_k, den += w_k; the colour is
 *        (float)(num / den), weight = (float)den, best_view = -1.  select 1, best: the colour is c_k of the largest w_k, ties go to the
 *        smaller k; best_view is that k and weight = (float)w_k of it; best_view = -1 where no view passed.
 *     6. Where used_bits == 0 the colour is the fallback row if fallback is given, else fill, and weight = 0.
 *     All outputs are written once by plain vector stores; no atomics: the outputs are bit-identical from run to run.  The look-up
 *     clamps its coordinate into the map before it converts it to an index and tests every index against the view's own height and
 *     width: no vertex (NaN, infinite, at a view's centre, far outside) makes it index outside a map.
 *   What the rule does NOT do: no occlusion test against the mesh itself (a vertex is tested against the panoramas' stored distances
 *     only); no texture atlas, colours are per vertex; no exposure matching between views; no wrap at the seam; more than 64 views are
 *     refused.
 *   Refusals.  K outside 0 .. 64; a map dimension below 1; tol negative or not finite; power outside 1 .. 8 with facing; select outside
 *     0 .. 1; facing with NULL normals; scale_log2 outside -200 .. 200; V above PERF_MESHCOLOR_MAX_VERTICES (2^30), F above
 *     PERF_MESHCOLOR_MAX_FACES (2^31 - 1), negative counts; NULL inputs or outputs where the count is positive, a NULL fill or
 *     bad_face_dev; facing other than 0 or 1; views_dev or color_maps_dev that is not 8-byte aligned. */
#ifndef PERF_HIP_MESHCOLOR_H
#define PERF_HIP_MESHCOLOR_H

#include "perf_hip_meshvis.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHCOLOR_ABI_VERSION 1
#define PERF_MESHCOLOR_MAX_VIEWS 64
#define PERF_MESHCOLOR_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHCOLOR_MAX_FACES 2147483647    /* 2^31 - 1 */
#define PERF_MESHCOLOR_MAX_POWER 8
#define PERF_MESHCOLOR_SELECT_BLEND 0
#define PERF_MESHCOLOR_SELECT_BEST 1

int perf_meshcolor_version(void); /* == PERF_MESHCOLOR_ABI_VERSION of the header the library was built from */

/* Stage A, the sums.  acc: device int64 [n_vertices, 3], zeroed by the call; bad_face_dev: device int64 [1].  vertices and acc may be
 * NULL when n_vertices is 0, faces when n_faces is 0. */
int perf_meshcolor_normal_sums(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int32_t scale_log2,
                               int64_t* acc, int64_t* bad_face_dev, void* stream);

/* Stage A, the unit normals fp32 [n_vertices, 3] of acc.  Both may be NULL when n_vertices is 0. */
int perf_meshcolor_normals(const int64_t* acc, int64_t n_vertices, float* normals, void* stream);

/* Stage B.  views_dev: DEVICE perf_meshvis_view [n_views]; color_maps_dev: DEVICE array of n_views device pointers, map k fp32
 * [height_k, width_k, 3]; view_sizes: HOST int32 [n_views, 2], the (height, width) the descriptors carry, for the refusals.  normals is
 * read only with facing != 0, power likewise; fallback: device fp32 [n_vertices, 3] or NULL; fill: HOST fp32 [3].  Per-vertex pointers
 * may be NULL when n_vertices is 0; views_dev, color_maps_dev and view_sizes when n_views is 0 (every vertex takes the fallback then). */
int perf_meshcolor_blend(const float* vertices, const float* normals, int64_t n_vertices, const perf_meshvis_view* views_dev,
                         const float* const* color_maps_dev, const int32_t* view_sizes, int32_t n_views, float tol, int32_t facing,
                         int32_t power, int32_t select, const float* fallback, const float* fill, float* colors, float* weight,
                         int64_t* used_bits, int8_t* best_view, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHCOLOR_H */
