/* Place the vertices of a mesh simplified by vertex clustering by quadric error, sums in fixed point: a fourteenth header of
 * libperf_hip.so, versioned on its own -- PERF_MESHQUADRIC_ABI_VERSION / perf_meshquadric_version(), recorded in
 * include/perf_hip_meshquadric.abi.json (`python tools/abi_digest.py --meshquadric [--write]`).  Error codes and conventions are those of
 * perf_hip.h: raw device pointers, 64-bit counts and a stream; an integer return code, the reason of a refusal in perf_last_error();
 * nothing is allocated and there is no workspace; everything that is refused is refused before anything is launched.  This header
 * includes no other unit's header: vertex_cluster, anchor and representative are what perf_meshsimp_cluster and perf_meshsimp_place
 * (placement 'mean') of perf_hip_meshsimp.h left, said in words.
 *
 * The statement.
 *   Inputs.
 *     vertices fp32 [V, 3] and faces int32 [F, 3].
 *     The grid of the clustering: origin lo [3] (fp32 values), cell edge h (fp32, finite, > 0), cells per axis n [3], 1 <= n <= 2^21.
 *     vertex_cluster int32 [V] and C, the labelling of the SAME vertices in the SAME grid (-1: a vertex that is not finite).
 *     anchor fp32 [C, 3]: the 'mean' placement.
 *     representative int32 [C]: a member of each cluster.
 *   Arithmetic.
 *     Everything is in double formed from the fp32 values.  Each operation rounds once and nothing is contracted.
 *     No square root and no division happen before a quantisation: only + - * / and llrint are used, so float64 arithmetic on any
 *     IEEE 754 machine reproduces every bit.
 *   The cell rule (that of perf_hip_meshsimp.h, restated).  Per axis:
 *       t = ((double)x - (double)lo) / (double)h,  then  t = min(max(t, 0), (double)n)       -- t clamped to [0, n] --
 *       i = min((int64)floor(t), n - 1)
 *       f = t - (double)i                                  (exact; 0 <= f <= 1, and f = 1 only for t = n)
 *     A finite vertex outside the grid is clamped into the border cell.
 *   Stage A, the sums (perf_meshquadric_sums).  Per face (a, b, c) with all indices in [0, V) and all three cluster ids in [0, C):
 *     1. e1 = (b - a) / h and e2 = (c - a) / h, per component.
 *          n = (e1y e2z - e1z e2y,  e1z e2x - e1x e2z,  e1x e2y - e1y e2x)
 *        n is unnormalised: a face weighs by its squared area in cell units, the weighting of out-of-core vertex clustering.
 *     2. The six products n_i n_j for ij in xx, xy, xz, yy, yz, zz and qA_ij = llrint(n_i n_j * 2^40), ties to even.
 *        If any n_i n_j * 2^40 is not finite or has magnitude >= 2^60, the face contributes nothing; the smallest index of such a face
 *        goes to skipped_face_dev (one 64-bit integer atomicMin per such face; -1 means none).  The flag is information, not a refusal.
 *     3. For each corner k of (a, b, c), with vertex p and cluster c_k:
 *          f = the cell fraction of p by the cell rule
 *          r = f - 0.5                                      (exact; -0.5 <= r <= 0.5)
 *          d = (n_x r_x + n_y r_y) + n_z r_z
 *          qb_i = llrint((n_i d) * 2^40)
 *        and the nine integers (qA_xx, qA_xy, qA_xz, qA_yy, qA_yz, qA_zz, qb_x, qb_y, qb_z) are added to row c_k of acc with 64-bit
 *        integer atomicAdd.  acc is int64 [C, 9], zeroed by the call.
 *        A face counts once per corner: a cluster that holds two of its corners gets it twice.  acc is the sum of per-vertex quadrics.
 *     4. A face with an index outside [0, V) is not followed; the smallest index of such a face goes to bad_face_dev (-1: none).
 *     5. A face with a cluster id of -1 (a vertex that is not finite), or any id outside [0, C), contributes nothing.
 *     The sums are integers: exact in any order and any grouping, bit-identical from run to run.  They wrap modulo 2^64 as int64 does:
 *     the qA terms are below 2^60, and |d| <= (|n_x| + |n_y| + |n_z|) / 2 puts the qb terms below 1.5 * 2^60, so eight such terms can
 *     already wrap; a lattice-sized face at a cell of 4 spacings (|n| near 2^-4) has terms near 2^32, and 2^30 of those fit.
 *   Stage B, the vertex (perf_meshquadric_place), one thread per cluster:
 *     1. A_ij = (double)acc_ij * 2^-40 and b_i likewise.  tr = (A_xx + A_yy) + A_zz.
 *        If tr is not > 0, the output row is anchor's row, bit for bit.
 *     2. i = the cell of vertices[representative] by the cell rule.  m_c = ((double)anchor_c - lo_c) / h - ((double)i_c + 0.5).
 *        A representative outside [0, V), or one with a coordinate that is not finite, gives the anchor's row.
 *     3. lambda = tr * 2^-10.  M = A + lambda I (lambda added to the three diagonal terms).  g_c = b_c + lambda m_c.
 *        This regularises towards the mean: on a plane the vertex is the mean moved onto the plane, on an edge it slides along the
 *        edge to the mean, at a corner it is the corner.
 *     4. The solve, by cofactors in this order:
 *          c00 = Myy Mzz - Myz Myz
 *          c01 = Mxz Myz - Mxy Mzz
 *          c02 = Mxy Myz - Mxz Myy
 *          c11 = Mxx Mzz - Mxz Mxz
 *          c12 = Mxy Mxz - Mxx Myz
 *          c22 = Mxx Myy - Mxy Mxy
 *          det = (Mxx c00 + Mxy c01) + Mxz c02
 *        If det is not > 0 or not finite, the output is the anchor's row.  Otherwise
 *          x_x = ((c00 g_x + c01 g_y) + c02 g_z) / det
 *          x_y = ((c01 g_x + c11 g_y) + c12 g_z) / det
 *          x_z = ((c02 g_x + c12 g_y) + c22 g_z) / det
 *        A component that is not finite gives the anchor's row.
 *     5. x_c = min(max(x_c, -0.5), 0.5): the vertex stays in its cell.
 *          p_c = (double)lo_c + (((double)i_c + 0.5) + x_c) * (double)h
 *        The output is (float)p_c.
 *   What the rule does NOT do: no face budget; no manifold repair; no boundary or feature constraints; no attribute quadrics (colours
 *     and normals still come from representative, unchanged); faces much larger than the cell are skipped by the 2^60 rule.
 *   Refusals.  NULL inputs or outputs where a count is positive; a NULL lo, bad_face_dev or skipped_face_dev; negative counts; V above
 *     2^30, F above 2^31 - 1, C above V; h not positive or not finite; lo not finite; a dimension outside 1 .. 2^21.
 *
 * Memory operations: return-less 64-bit vector atomics (integer atomicAdd, atomicMin) and plain vector stores; no floating-point atomics
 *   anywhere.  One thread per face in face order; a face whose three corners share a cluster adds its three corners' integers in
 *   registers and sends 9 atomics, not 27; two corners that share one go together (18).  Such whole faces that follow one another along
 *   a wave with one cluster (surface-nets order makes such runs) are summed inside the wave by a segmented scan and the run's last lane
 *   sends the nine sums; a term that is zero is not sent.  All of it regroups integer sums: the outcome is the same to the bit.  The
 *   shape that serialises is every lane on one 72-byte row: the runs make it one lane per wave.  No scratch; no thread waits on
 *   another. */
#ifndef PERF_HIP_MESHQUADRIC_H
#define PERF_HIP_MESHQUADRIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHQUADRIC_ABI_VERSION 1
#define PERF_MESHQUADRIC_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHQUADRIC_MAX_FACES 2147483647    /* 2^31 - 1 */
#define PERF_MESHQUADRIC_MAX_CELLS 2097152       /* 2^21, per axis */
#define PERF_MESHQUADRIC_TERMS 9                 /* per cluster: qA xx, xy, xz, yy, yz, zz, then qb x, y, z */
#define PERF_MESHQUADRIC_FRACTION_BITS 40        /* the sums' fixed point */
#define PERF_MESHQUADRIC_SKIP_BITS 60            /* a product times 2^40 at or above 2^60 skips its face */
#define PERF_MESHQUADRIC_REGULARISER_BITS 10     /* lambda = tr * 2^-10 */

int perf_meshquadric_version(void); /* == PERF_MESHQUADRIC_ABI_VERSION of the header the library was built from */

/* Stage A.  lo: HOST fp32 [3]; nx, ny, nz: the cells per axis.  acc: device int64 [n_clusters, 9], zeroed by the call; bad_face_dev,
 * skipped_face_dev: device int64 [1] each.  vertices and vertex_cluster may be NULL when n_vertices is 0, faces when n_faces is 0, acc
 * when n_clusters is 0. */
int perf_meshquadric_sums(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* lo, float h,
                          int32_t nx, int32_t ny, int32_t nz, const int32_t* vertex_cluster, int64_t n_clusters, int64_t* acc,
                          int64_t* bad_face_dev, int64_t* skipped_face_dev, void* stream);

/* Stage B.  anchor: device fp32 [n_clusters, 3]; representative: device int32 [n_clusters]; acc: what perf_meshquadric_sums left;
 * cluster_vertices: device fp32 [n_clusters, 3] (it may be anchor itself: a thread reads its row before it writes it).  vertices may
 * be NULL when n_vertices is 0; anchor, representative, acc and cluster_vertices when n_clusters is 0. */
int perf_meshquadric_place(const float* vertices, int64_t n_vertices, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz,
                           const float* anchor, const int32_t* representative, const int64_t* acc, int64_t n_clusters,
                           float* cluster_vertices, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHQUADRIC_H */
