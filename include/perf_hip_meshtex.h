/* Bake a texture atlas for a triangle mesh from the registered panoramas: a thirteenth header of libperf_hip.so, versioned on its own --
 * PERF_MESHTEX_ABI_VERSION / perf_meshtex_version(), recorded in include/perf_hip_meshtex.abi.json (`python tools/abi_digest.py --meshtex
 * [--write]`).  Error codes and conventions are those of perf_hip.h: raw device pointers, counts and a stream; an integer return code, the
 * reason of a refusal in perf_last_error(); nothing is allocated and there is no workspace; everything that is refused is refused before
 * anything is launched.  This header includes no other unit's header: views_dev is a const void* that points at the DEVICE
 * perf_meshvis_view [n_views] array of perf_hip_meshvis.h, unchanged, as perf_meshcolor_blend takes it.
 *
 * The statement.
 *   The layout is closed form: no packing search, nothing data dependent, no atomics but the flag's.
 *   Tiles and capacity.
 *     The atlas is a square image S x S, 64 <= S <= 16384 (size), cut into tiles of edge T texels, 4 <= T <= S (tile).
 *     n = S / T tiles fit per row (integer division); the margin beyond n T is unused.
 *     A tile holds two faces: face f lives in tile t = f >> 1 as half h = f & 1.
 *     The tile origin is (X0, Y0) = ((t % n) T, (t / n) T).
 *     Capacity is 2 n^2 faces; more faces than that are refused.
 *   Corners.
 *     m = T - 3.  Corner texel indices as (column, row):
 *       h = 0:  a (X0, Y0),  b (X0 + m, Y0),  c (X0, Y0 + m)
 *       h = 1:  the same rotated 180 degrees about the tile centre:
 *               a (X0 + T - 1, Y0 + T - 1),  b (X0 + T - 1 - m, Y0 + T - 1),  c (X0 + T - 1, Y0 + T - 1 - m)
 *     A corner at texel (i, j) has u = (i + 0.5) / S, v = (j + 0.5) / S in fp32 (the sum is exact, the quotient rounds once); when S is a
 *     power of two both are exact: a corner sits on a texel centre.  Texel (i, j) is element j S + i of every per-texel array: v grows
 *     with the row index.
 *   Which face owns a texel.
 *     A texel with local index (i, j) in its tile belongs to half h = (i + j >= T).
 *     For h = 1 the local index is mirrored: (li, lj) = (T - 1 - i, T - 1 - j); for h = 0 (li, lj) = (i, j).
 *     Half 0 therefore owns li + lj <= m + 2 and half 1 owns li + lj <= m + 1: every texel of a used tile has exactly one owner.
 *     Coverage codes: 0 no face (the margin, a tile beyond the faces, the absent half 1 of the last tile of an odd count, a face with an
 *     index outside [0, V)); 1 li + lj <= m, inside the triangle; 2 gutter.
 *   Barycentrics and the texel's point.
 *     beta = li / m, gamma = lj / m in DOUBLE; alpha = (1 - beta) - gamma.
 *     In the gutter they are EXTRAPOLATED, NOT CLAMPED: the texel's point lies in the face's plane just outside the triangle, and alpha
 *     can be negative there.
 *     Per component, in double from the fp32 vertices, one rounding per operation, nothing contracted:
 *       P = (a + beta (b - a)) + gamma (c - a),  rounded to fp32 once.
 *     A function linear in the barycentrics is then reproduced by bilinear sampling at every point of the triangle: the four taps with
 *     a non-zero weight are texels the face owns; legs and hypotenuse all carry m + 1 uniformly spaced samples, so the two sides of a
 *     shared edge sample the same 3-D points.
 *   The texel's normal.
 *     With normals == NULL it is the face's own: e1 = b - a, e2 = c - a,
 *       n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)  in double as stage A of perf_hip_meshcolor.h writes it,
 *       len = sqrt((nx nx + ny ny) + nz nz),  normal_c = (float)(n_c / len),  and exactly 0 where len == 0.
 *     With per-vertex normals fp32 [V, 3] it is (alpha Na + beta Nb) + gamma Nc in double, rounded once and NOT normalised: the blend
 *     divides by its length.
 *   perf_meshtex_points, the materialised route, stores per texel: points, point_normals, face_of (int32, -1: no face), coverage.  A
 *     texel with no face gets point 0, normal 0, face_of = -1, coverage 0.  A face with an index outside [0, V) contributes nothing:
 *     its texels are texels of no face, and the smallest index of such a face is left in bad_face_dev (-1: none) by one 64-bit integer
 *     atomicMin per such face.
 *   perf_meshtex_bake, the fused bake: one thread per texel forms the point and the normal above in registers, rounds them to fp32
 *     exactly as perf_meshtex_points stores them, and takes them through STAGE B OF perf_hip_meshcolor.h, UNCHANGED: the same look-up,
 *     depth test, facing test, weights, selection and order of the views (one device function, which perf_meshcolor_blend runs too).
 *     image, weight and used_bits of a covered texel are therefore bit for bit the colors, weight and used_bits perf_meshcolor_blend
 *     gives at points / point_normals.  With facing == 0 the normal is not read.  Where no view passes: with fallback fp32 [V, 3] the
 *     colour is the per-vertex rows interpolated, (alpha Ca + beta Cb) + gamma Cc in double, rounded once; without it, fill.  Texels of
 *     no face take fill, weight 0, bits 0, coverage 0.  All outputs are plain vector stores written once: runs are bit-identical.  A
 *     wave covers an 8 x 8 block of texels (at T = 8 it reads two faces); the views and the map pointers are staged in LDS.
 *   What the rule does NOT do: every face gets the same texel budget -- no area-proportional charts, no chart merging; no mip-safe
 *     padding between tiles; no exposure matching between views; no occlusion test against the mesh itself; no wrap at the seam; more
 *     than 64 views are refused.
 *   Refusals.  S outside 64 .. 16384; T below 4 or above S; F above 2 n^2; V above PERF_MESHTEX_MAX_VERTICES (2^30); negative counts;
 *     K outside 0 .. 64; a map dimension below 1; tol negative or not finite; facing other than 0 or 1; power outside 1 .. 8 with
 *     facing; select outside 0 .. 1; NULL inputs where the count is positive, NULL outputs, a NULL fill or bad_face_dev; views_dev or
 *     color_maps_dev that is not 8-byte aligned. */
#ifndef PERF_HIP_MESHTEX_H
#define PERF_HIP_MESHTEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHTEX_ABI_VERSION 1
#define PERF_MESHTEX_MIN_SIZE 64
#define PERF_MESHTEX_MAX_SIZE 16384
#define PERF_MESHTEX_MIN_TILE 4
#define PERF_MESHTEX_MAX_VIEWS 64
#define PERF_MESHTEX_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHTEX_MAX_POWER 8
#define PERF_MESHTEX_COVER_NONE 0
#define PERF_MESHTEX_COVER_INSIDE 1
#define PERF_MESHTEX_COVER_GUTTER 2

int perf_meshtex_version(void); /* == PERF_MESHTEX_ABI_VERSION of the header the library was built from */

/* The corner UVs.  uv: device fp32 [n_faces, 3, 2], (u, v) of corners a, b, c.  uv may be NULL when n_faces is 0. */
int perf_meshtex_uv(int64_t n_faces, int32_t size, int32_t tile, float* uv, void* stream);

/* The materialised route.  vertices fp32 [n_vertices, 3]; normals fp32 [n_vertices, 3] or NULL (the face's own normal); faces int32
 * [n_faces, 3]; points, point_normals: device fp32 [size * size, 3]; face_of: device int32 [size * size]; coverage: device uint8
 * [size * size]; bad_face_dev: device int64 [1].  vertices may be NULL when n_vertices is 0, faces when n_faces is 0. */
int perf_meshtex_points(const float* vertices, int64_t n_vertices, const float* normals, const int32_t* faces, int64_t n_faces, int32_t size,
                        int32_t tile, float* points, float* point_normals, int32_t* face_of, uint8_t* coverage, int64_t* bad_face_dev,
                        void* stream);

/* The fused bake.  views_dev: DEVICE perf_meshvis_view [n_views] (perf_hip_meshvis.h); color_maps_dev: DEVICE array of n_views device
 * pointers, map k fp32 [height_k, width_k, 3]; view_sizes: HOST int32 [n_views, 2], the (height, width) the descriptors carry, for the
 * refusals; the three may be NULL when n_views is 0 (every texel takes the fallback then).  fallback: device fp32 [n_vertices, 3] or
 * NULL; fill: HOST fp32 [3].  image: device fp32 [size, size, 3]; weight: device fp32 [size, size]; used_bits: device int64 [size, size];
 * coverage: device uint8 [size, size]; bad_face_dev: device int64 [1]. */
int perf_meshtex_bake(const float* vertices, int64_t n_vertices, const float* normals, const int32_t* faces, int64_t n_faces, int32_t size,
                      int32_t tile, const void* views_dev, const float* const* color_maps_dev, const int32_t* view_sizes, int32_t n_views,
                      float tol, int32_t facing, int32_t power, int32_t select, const float* fallback, const float* fill, float* image,
                      float* weight, int64_t* used_bits, uint8_t* coverage, int64_t* bad_face_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHTEX_H */
