/* Cull the faces of a triangle mesh no registered panorama saw -- vertex bits, face rule, compaction by a face mask: a ninth header of
 * libperf_hip.so, versioned on its own -- PERF_MESHVIS_ABI_VERSION / perf_meshvis_version(), recorded in include/perf_hip_meshvis.abi.json
 * (`python tools/abi_digest.py --meshvis [--write]`).  Error codes and conventions are those of perf_hip.h: raw device pointers, counts
 * and a stream; an integer return code, the reason of a refusal in perf_last_error(); a caller-owned workspace sized by
 * perf_meshvis_workspace_bytes; nothing is allocated; everything that is refused is refused before anything is launched.
 *
 * The statement.  A view is a registered panorama: the pose's R^T and centre t (PanoFrame of perf_pano_reproject), the height and width
 *   of its masked distance map and the map itself, fp32 [H, W] = distance_map * mask (0 where the panorama stored nothing).  K <= 64 views
 *   of ANY sizes are given as a device array of perf_meshvis_view.
 *   Stage 1, perf_meshvis_vertex_bits.  vertices fp32 [V, 3] -> visible_bits, free_bits int64 [V]; bit k belongs to view k, bits >= K
 *     are 0.  For vertex p and view k, dist = |R^T (p - t)| and proj = the bilinear look-up of the map along that direction, by THE
 *     ARITHMETIC OF perf_pano_reproject's kernel RESTATED LINE FOR LINE: fp32, one rounding per operation in the same order, asinf /
 *     atan2f, grid_sample's align_corners=False coordinate with the border clamp, the nw / ne / sw / se accumulation order.
 *       visible_k  <=>  dist < proj + tol            (the reference's mode-0 test, nerf.py:321-358, whose tol is 1/256)
 *       free_k     <=>  dist < proj + (-free_tol)    (the vertex lies in front of what view k stored by more than the band)
 *     so bit k of visible_bits (free_bits) is, to the bit, what perf_pano_reproject leaves in a zeroed mask in mode 0 with eps = tol
 *     (eps = -free_tol).  A pixel the panorama did not store has proj = 0 and makes a vertex neither visible nor free; so does a NaN.
 *     The look-up clamps its coordinate into the map before it converts it to an index and tests every index against the view's own
 *     height and width: no vertex (NaN, infinite, at a view's centre, far outside) makes it index outside a map.
 *     One thread per vertex, looping over the views, which a workgroup stages in LDS with the 256 vertices it takes; both words are
 *     written once by plain vector stores; no atomics.
 *   Stage 2, perf_meshvis_face_keep.  faces int32 [F, 3] -> face_keep uint8 [F].  For a face (a, b, c), M = the low K bits:
 *       bits = visible[a] & visible[b] & visible[c] & M.
 *     With facing, bit k stays only where the face points at view k's centre t_k, all in DOUBLE formed from the fp32 values, one
 *     rounding per operation, nothing contracted:
 *       e1 = b - a, e2 = c - a                                        (per component)
 *       n  = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)
 *       g  = t_k - a
 *       s  = (n.x g.x + n.y g.y) + n.z g.z
 *     and the face points at view k iff s > 0 (a NaN or a degenerate face points at nobody).  Surface-nets normals point from the dense
 *     side to the empty side, so the skin a camera inside a room saw points at it.
 *     keep = popcount(bits) >= min_views, and, with carve, ((free[a] | free[b] | free[c]) & M) == 0.
 *     A face with an index outside [0, V) is never followed and gets 0; the smallest index of such a face is left in bad_face_dev (-1:
 *     none; one integer atomicMin per such face, no other atomic), which the caller reads with the counts of stage 3.
 *   Stage 3, perf_meshvis_filter_count / _write: compaction by ANY face mask.  A face is kept iff face_keep is nonzero and its three
 *     indices are in [0, V) (such a face is dropped silently here: stage 2 and perf_meshcc_label name it).  A vertex is kept iff a kept
 *     face names it.  Kept vertices and faces keep their relative order, faces are re-indexed, kept_vertex_index int32 [V'] maps new
 *     vertices to old ones, so per-vertex attributes are carried by one gather.  Kept faces mark their vertices with plain same-value
 *     stores; the ranks come from two scans (groups of 256); no atomics: the outputs are bit-identical from run to run.
 *   What the rule does NOT do: no occlusion test against the mesh itself (a vertex is tested against the panoramas' stored distances
 *     only); no colours are taken from the panoramas; more than 64 views are refused.
 *   Refusals.  K outside 0 .. PERF_MESHVIS_MAX_VIEWS; a map dimension < 1; tolerances that are negative or not finite; V above
 *     PERF_MESHVIS_MAX_VERTICES (2^30: vertex indices are int32); F above PERF_MESHVIS_MAX_FACES (2^38: face counters and offsets are
 *     64-bit); min_views < 1; NULL pointers; a short or misaligned workspace; negative capacities, and capacities below the counted totals.
 *
 * Protocol.  vertex_bits -> face_keep -> filter_count -> the caller reads (V', F') and the flag of stage 2, THE ONE HOST READ-BACK, and
 *   allocates -> filter_write.
 *
 * Workspace (stage 3 only), in 8-byte words.  L(n) = n_1 + n_2 + ... with n_1 = ceil(n / 256), n_{k+1} = ceil(n_k / 256), down to the
 * level of one word; S(n) = 0 for n = 0 and G + L(G) with G = ceil(n / 256) otherwise (the counts of groups of 256 items and their scan).
 * perf_meshvis_workspace_bytes = 8 * ((ceil(V / 2) + S(V) + S(F) + 4) rounded up to an even number): one int32 array [V] (the marks of
 * the kept faces' vertices, then the kept vertices' new indices), the vertices' and the faces' group counts, four totals.  4 bytes per
 * vertex and 1/32 byte per face, and the levels. */
#ifndef PERF_HIP_MESHVIS_H
#define PERF_HIP_MESHVIS_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHVIS_ABI_VERSION 1
#define PERF_MESHVIS_MAX_VIEWS 64
#define PERF_MESHVIS_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHVIS_MAX_FACES 274877906944  /* 2^38 */

/* One registered panorama, 64 bytes, 8-byte aligned: an array of them lives ON THE DEVICE. */
typedef struct perf_meshvis_view {
    float rt[9];                 /* R^T of the pose, row major */
    float t[3];                  /* the camera centre */
    int32_t height, width;       /* of distance_map */
    const float* distance_map;   /* device fp32 [height, width]: distance_map * mask */
} perf_meshvis_view;

int perf_meshvis_version(void);          /* == PERF_MESHVIS_ABI_VERSION of the header the library was built from */
int64_t perf_meshvis_sizeof_view(void);  /* == sizeof(perf_meshvis_view) */

/* Bytes of the one workspace that serves filter_count and filter_write of a mesh of n_vertices and n_faces (a multiple of 16); -1 with a
 * reason: a negative count, n_vertices above PERF_MESHVIS_MAX_VERTICES, n_faces above PERF_MESHVIS_MAX_FACES. */
int64_t perf_meshvis_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Stage 1.  views_dev: DEVICE perf_meshvis_view [n_views]; view_sizes: HOST int32 [n_views, 2], the (height, width) the descriptors
 * carry, for the refusals (the kernel bounds its indices by the descriptors' own).  vertices, visible_bits and free_bits may be NULL when
 * n_vertices is 0; views_dev and view_sizes when n_views is 0 (every bit is 0 then). */
int perf_meshvis_vertex_bits(const float* vertices, int64_t n_vertices, const perf_meshvis_view* views_dev, const int32_t* view_sizes,
                             int32_t n_views, float tol, float free_tol, int64_t* visible_bits, int64_t* free_bits, void* stream);

/* Stage 2.  centres: device fp32 [n_views, 3], read only with facing != 0 (NULL otherwise is fine); free_bits is read only with
 * carve != 0.  bad_face_dev: device int64 [1].  Inputs and face_keep may be NULL when n_faces is 0. */
int perf_meshvis_face_keep(const int32_t* faces, int64_t n_faces, const float* vertices, int64_t n_vertices, const int64_t* visible_bits,
                           const int64_t* free_bits, const float* centres, int32_t n_views, int32_t facing, int32_t min_views, int32_t carve,
                           uint8_t* face_keep, int64_t* bad_face_dev, void* stream);

/* Stage 3, count: face_keep uint8 [n_faces] (nonzero = kept) -> the kept vertices' new indices in the workspace and counts_dev [2] int64
 * ON THE DEVICE: (V', F').  faces and face_keep may be NULL when n_faces is 0. */
int perf_meshvis_filter_count(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const uint8_t* face_keep, void* workspace,
                              int64_t workspace_bytes, int64_t* counts_dev, void* stream);

/* Stage 3, write: faces_out int32 [F', 3], kept_vertex_index int32 [V'] and, unless vertices is NULL, vertices_out fp32 [V', 3] of the
 * SAME faces, face_keep and workspace perf_meshvis_filter_count was given (the stream's order puts it after the count).  vertex_capacity /
 * face_capacity: rows the arrays hold; capacities below the counted totals are refused: the call reads the totals back from the workspace
 * after the stream has drained, so it is not for stream capture.  Outputs may be NULL when their capacity is 0; vertices_out must not be
 * NULL when vertices is not and vertex_capacity > 0. */
int perf_meshvis_filter_write(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const uint8_t* face_keep, const float* vertices,
                              const void* workspace, int64_t workspace_bytes, float* vertices_out, int32_t* kept_vertex_index,
                              int64_t vertex_capacity, int32_t* faces_out, int64_t face_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHVIS_H */
