/* Simplify a triangle mesh on the device by vertex clustering -- cells, clusters, positions, representatives, remapped and de-duplicated
 * faces: a tenth header of libperf_hip.so, versioned on its own -- PERF_MESHSIMP_ABI_VERSION / perf_meshsimp_version(), recorded in
 * include/perf_hip_meshsimp.abi.json (`python tools/abi_digest.py --meshsimp [--write]`).  Error codes and conventions are those of
 * perf_hip.h: raw device pointers, 64-bit counts and a stream; an integer return code, the reason of a refusal in perf_last_error(); a
 * caller-owned workspace sized by perf_meshsimp_workspace_bytes; nothing is allocated; everything that is refused is refused before
 * anything is launched.
 *
 * The statement.  Inputs: vertices fp32 [V, 3], faces int32 [F, 3] and a grid: origin lo [3] (fp32 values), cell edge h (fp32, finite,
 *   > 0), cells per axis n [3] with 1 <= n <= 2^21.  V <= 2^30, F <= 2^31 - 1.
 *   The cell rule.  Per axis, in double formed from the fp32 values, one rounding per operation, nothing contracted:
 *       t = ((double)x - (double)lo) / (double)h,  then  t = min(max(t, 0), (double)n)
 *       i = min((int64)floor(t), n - 1)
 *       f = t - (double)i                                  (exact; 0 <= f <= 1, and f = 1 only for t = n)
 *       q = llrint(f * 2^32)                               (ties to even; 0 <= q <= 2^32)
 *       key = ix << 42 | iy << 21 | iz
 *     A finite vertex outside the grid is clamped into the border cell.  A vertex with a coordinate that is not finite joins nothing (its
 *     vertex_cluster is -1); the smallest index of such a vertex is left in a device flag, which the caller reads with the counts and
 *     refuses the mesh by.
 *   Clusters.  A cluster is the set of the vertices with one key.  Its id is the rank of its smallest member index among all clusters'
 *     smallest member indices: ids run 0 .. C-1 and depend on no race.  vertex_cluster int32 [V].
 *   Position, 'mean'.  S = the int64 sum of q over the members, per axis (at most 2^30 * 2^32: it fits);
 *       m = (double)S / ((double)count * 4294967296.0)          -- S / (count * 2^32) --
 *       p = (double)lo + ((double)i + m) * (double)h
 *     and the cluster's vertex is (float)p.  The sums are integers: exact in any order.  p lies within h * 2^-32 of the mean of the
 *     members (as the cell rule places them) before the final rounding.
 *   Representative  int32 [C]: the member that minimises d2 = (dx dx + dy dy) + dz dz, dx = (double)x - p_x (the double p), in double,
 *     one rounding per operation; ties go to the smaller index.  placement 'member' puts the cluster's vertex at
 *     vertices[representative], bit for bit: no shrinkage, every output vertex is an input vertex.  Under either placement
 *     representative is what carries per-vertex attributes.
 *   Faces.  A face (a, b, c) becomes (cluster[a], cluster[b], cluster[c]).  A face with an index outside [0, V) is never followed (it
 *     is written as (-1, -1, -1) and not kept); the smallest index of such a face is left in a device flag that the caller reads with the
 *     counts.  A face is dropped when two of its three cluster ids are equal (or one is -1).  dedupe 'oriented': among the faces whose
 *     triples are equal up to rotation only the one with the smallest face index stays; 'unoriented': among the faces whose triples are
 *     equal as sets only the smallest face index stays, and it keeps its own winding (the choice for a double skin thinner than a cell);
 *     none: every face that is not degenerate stays.  The outcome is face_keep uint8 [F] beside the remapped faces int32 [F, 3].
 *   Compaction (the caller's: perf_meshvis_filter_count / _write on the remapped faces and face_keep, include/perf_hip_meshvis.h).
 *     Clusters no kept face names are dropped, surviving clusters and faces keep their relative order (cluster-id order, face order),
 *     faces are re-indexed, kept_vertex_index int32 [V'] holds the surviving clusters' representatives.
 *   What the rule does NOT do: no manifold repair (clustering can pinch a surface: two sheets that pass through one cell share its
 *     vertex, an edge may end with more than two faces); no quadric error placement; no face budget; no colours are taken from anywhere
 *     but the representatives; more than 2^21 cells per axis are refused.
 *
 * The two hash sets.  Both are wait-free sets of int32 member indices in a table of T(n) uint32 slots, T(n) = the smallest power of two
 *   >= max(2 n, 256), so there are always more empty slots than keys.  A slot is EMPTY (0xffffffff) or holds the smallest index seen so
 *   far among the members of ONE key.  A thread with member i and key k probes linearly from hash(k): on an EMPTY slot it does
 *   atomicCAS(EMPTY -> i); when the compare-and-swap fails it goes on FROM THE VALUE THE COMPARE-AND-SWAP RETURNED; on an occupied slot it
 *   compares k with the occupant's key, which it reads from an immutable array an EARLIER launch wrote (the vertices' keys; the remapped
 *   faces), never from the table; if the keys are equal it does atomicMin(slot, i), remembers the slot and stops, else it moves to the
 *   next slot.
 *   Why the outcome depends on no race.  (1) A slot changes EMPTY -> j once, by a compare-and-swap, and afterwards only by atomicMin of
 *     members of j's key: a thread does atomicMin only after it has seen an occupant of its own key, and every later value of the slot is a
 *     member of that key.  So a slot belongs to one key for good, whichever occupant a thread happened to read.  (2) Two slots never
 *     belong to one key: a thread claims an EMPTY slot for k only after it has passed every slot from hash(k) on and found each to belong
 *     to another key (for good, by 1); a second thread of key k walks the same slots in the same order, passes the same ones and stops at
 *     the first that is EMPTY or k's -- the same slot, since that slot is not EMPTY any more.  (3) Every member of k ends with
 *     min(slot, i) applied to k's slot -- by its compare-and-swap or its atomicMin -- and min is commutative: after the launch the slot holds
 *     the smallest member of k, whoever won what.  Termination: a walk passes only slots of other keys, of which there are fewer than T:
 *     it ends within T steps whatever the other threads do.  No thread waits for another thread's progress, no value is polled.
 *   The hash functions.  M = 0x9E3779B97F4A7C15, b = log2 T, all arithmetic modulo 2^64:
 *       cells:  hash(key) = (key * M) >> (64 - b)
 *       faces:  hash(a, b', c) = ((((uint64)a << 32 | b') * M) >> (64 - b)) + c) & (T - 1)      of the canonical triple (a, b', c):
 *     'oriented' the rotation of the remapped face that puts its smallest id first, 'unoriented' the three ids ascending.
 *   The vertices of a wave that follow one another with one key (surface-nets order makes such runs long) send one member, the run's
 *   first, to the table; the sums of q and the minima of d2 are reduced over such runs inside the wave, and the waves' runs joined across
 *   a workgroup of 1,024 vertices, before they touch memory (integers and minima: exact in any grouping).
 *
 * Memory operations: vector atomics (atomicCAS, atomicMin, integer atomicAdd) and plain vector stores; no floating-point atomics
 *   anywhere: every output is bit-identical from run to run.
 *
 * Protocol.  [bounds, when the caller has no box -> the caller reads six floats: one more read-back] -> cluster -> faces -> the caller's
 *   perf_meshvis_filter_count -> the caller reads (C, the vertex flag, the face flag, V', F'): THE ONE HOST READ-BACK of a simplification
 *   beside the one perf_meshvis_filter_write makes of its own totals -> the caller allocates -> place -> perf_meshvis_filter_write.
 *   Used apart, cluster -> read (C, flag) -> place makes one read-back and faces -> read (flag) one.
 *
 * Workspace.  L(n) = n_1 + n_2 + ... with n_1 = ceil(n / 256), n_{k+1} = ceil(n_k / 256), down to the level of one word; S(n) = 0 for
 *   n = 0 and G + L(G) with G = ceil(n / 256) otherwise.  perf_meshsimp_workspace_bytes = 16 V + 4 T(V) + 4 F' + 4 T(F) + 8 S(V) + 32
 *   rounded up to a multiple of 16, with F' = F rounded up to an even number: the vertices' keys (8 bytes each), their slots, then ranks (4), their clusters' smallest
 *   members (4), the cells' table; the faces' slots (4) and the faces' table; the vertices' group counts and their scan; four totals.
 *   24 to 32 bytes per vertex and 12 to 20 bytes per face, and the levels.  perf_meshsimp_place takes a scratch array of its own,
 *   48 bytes per cluster (three sums, then the double p; the count; the key; the smallest d2). */
#ifndef PERF_HIP_MESHSIMP_H
#define PERF_HIP_MESHSIMP_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHSIMP_ABI_VERSION 1
#define PERF_MESHSIMP_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHSIMP_MAX_FACES 2147483647    /* 2^31 - 1 */
#define PERF_MESHSIMP_MAX_CELLS 2097152       /* 2^21, per axis */
#define PERF_MESHSIMP_PLACE_MEAN 0
#define PERF_MESHSIMP_PLACE_MEMBER 1
#define PERF_MESHSIMP_DEDUPE_NONE 0
#define PERF_MESHSIMP_DEDUPE_ORIENTED 1
#define PERF_MESHSIMP_DEDUPE_UNORIENTED 2

int perf_meshsimp_version(void);          /* == PERF_MESHSIMP_ABI_VERSION of the header the library was built from */

/* T(n) of the comment above: the slots of the table of a set of n members; -1 with a reason for a negative n or one above 2^31 - 1. */
int64_t perf_meshsimp_table_slots(int64_t n);

/* Bytes of the one workspace that serves cluster and faces of a mesh of n_vertices and n_faces (a multiple of 16); -1 with a reason: a
 * negative count, n_vertices above PERF_MESHSIMP_MAX_VERTICES, n_faces above PERF_MESHSIMP_MAX_FACES. */
int64_t perf_meshsimp_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* bounds_dev fp32 [6] ON THE DEVICE: the smallest x, y, z and the largest x, y, z among the finite coordinates of vertices fp32
 * [n_vertices, 3] (integer atomicMin / atomicMax on an order-preserving image of the floats); (+inf x 3, -inf x 3) when there is none.
 * vertices may be NULL when n_vertices is 0. */
int perf_meshsimp_bounds(const float* vertices, int64_t n_vertices, float* bounds_dev, void* stream);

/* vertex_cluster int32 [n_vertices] and counts_dev [2] int64 ON THE DEVICE: (C, the smallest index of a vertex with a coordinate that is
 * not finite, or -1).  lo: HOST fp32 [3]; nx, ny, nz: the cells per axis.  vertices and vertex_cluster may be NULL when n_vertices is 0.
 * workspace: 16-byte aligned, >= workspace_bytes(n_vertices, n_faces); n_faces only places the arrays in it. */
int perf_meshsimp_cluster(const float* vertices, int64_t n_vertices, int64_t n_faces, const float* lo, float h, int32_t nx, int32_t ny,
                          int32_t nz, int32_t* vertex_cluster, int64_t* counts_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* cluster_vertices fp32 [n_clusters, 3] and representative int32 [n_clusters] of the labelling vertex_cluster [n_vertices] of the SAME
 * vertices and grid; placement: PERF_MESHSIMP_PLACE_MEAN or _MEMBER.  scratch: device, 16-byte aligned, >= 48 * n_clusters bytes.
 * Ids outside [0, n_clusters) are skipped.  Everything may be NULL when n_clusters is 0. */
int perf_meshsimp_place(const float* vertices, int64_t n_vertices, const float* lo, float h, int32_t nx, int32_t ny, int32_t nz,
                        const int32_t* vertex_cluster, int64_t n_clusters, int32_t placement, float* cluster_vertices, int32_t* representative,
                        void* scratch, int64_t scratch_bytes, void* stream);

/* faces int32 [n_faces, 3] -> faces_out int32 [n_faces, 3] (the cluster ids), face_keep uint8 [n_faces] and bad_face_dev int64 [1] ON THE
 * DEVICE (the smallest index of a face with an index outside [0, n_vertices), or -1).  dedupe: PERF_MESHSIMP_DEDUPE_*.  The stream's order
 * puts it after the cluster that wrote vertex_cluster; the same workspace may serve both.  faces, faces_out and face_keep may be NULL when
 * n_faces is 0, vertex_cluster when n_vertices is 0. */
int perf_meshsimp_faces(const int32_t* faces, int64_t n_faces, const int32_t* vertex_cluster, int64_t n_vertices, int32_t dedupe,
                        int32_t* faces_out, uint8_t* face_keep, int64_t* bad_face_dev, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHSIMP_H */
