/* Connected components of a triangle mesh on the device -- label, count, select, compact: an eighth header of libperf_hip.so, versioned
 * on its own -- PERF_MESHCC_ABI_VERSION / perf_meshcc_version(), recorded in include/perf_hip_meshcc.abi.json
 * (`python tools/abi_digest.py --meshcc [--write]`).  Error codes and conventions are those of perf_hip.h: raw device pointers, counts
 * and a stream; an integer return code, the reason of a refusal in perf_last_error(); a caller-owned workspace sized by
 * perf_meshcc_workspace_bytes; nothing is allocated; everything that is refused is refused before anything is launched.
 *
 * The statement.  Inputs: faces int32 [F, 3] and the number of vertices V.
 *   Connectivity.  Two vertices are connected when a face names both; components are the classes of the transitive closure.
 *     Connectivity is by INDEX, not by position.  A vertex in no face is a component of its own with 0 faces.  Faces with repeated
 *     indices are legal (they connect what they name and count as faces).
 *   Component ids.  The id of a component is the rank of its smallest vertex index among all components' smallest vertex indices: ids
 *     run 0 .. C-1 and depend neither on the order of the faces nor on any race.
 *   vertex_component  int32 [V]: the id of each vertex's component.
 *   faces_per_component  int64 [C]: a face belongs to the component of its vertices.
 *   vertices_per_component  int32 [C].
 *   signed_volume  float64 [C]: the sum over the component's faces (a, b, c) of a . (b x c) / 6, each term formed in double from the
 *     fp32 vertices; positive for a closed surface whose normals point outward.  IT IS THE ONE OUTPUT THAT MAY DEPEND ON THE ORDER OF
 *     SUMMATION IN ITS LAST BITS (terms are added with floating-point atomics); every other output is exact and identical from run
 *     to run.
 *   Selection (the caller's: perf_amd.mesh.select_components).  Component c is kept iff faces[c] >= min_faces, and keep_largest is
 *     None or the rank of c by (more faces first, then lower id) is below keep_largest, and orientation is None, or 'inward' and
 *     signed_volume[c] < 0, or 'outward' and signed_volume[c] > 0.  The library takes the outcome as keep uint8 [C].
 *   Filtering.  Kept vertices keep their relative order; kept faces (all of a face's vertices are kept or none are) keep their relative
 *     order and are re-indexed; kept_vertex_index int32 [V'] maps new vertices to old ones, so per-vertex attributes are carried by one
 *     gather.  The ranks come from a scan: the outputs are bit-identical from run to run.
 *   Refusals.  V <= PERF_MESHCC_MAX_VERTICES (2^30, the mesh ABI's ceiling); F <= PERF_MESHCC_MAX_FACES, above 2^31: face counters and
 *     offsets are 64-bit.  A face with an index outside [0, V) is never followed: no kernel reads or writes outside its arrays because
 *     of it (every kernel checks the three indices of a face before it uses them, and a component id before it indexes with it); the
 *     labelling raises a device flag -- the smallest index of such a face -- that the caller reads with the component count.
 *
 * The labelling: a wait-free union-find.  Vertices are ORDERED by key(x), a fixed bijection of the 32-bit words that scatters
 *   neighbouring indices (x < y below means key(x) < key(y)): hooking by index would turn a strip whose indices ascend along it -- every
 *   surface-nets mesh -- into one chain as long as the strip.  parent [V] (stored as keys) starts as the identity.  INVARIANT:
 *   parent[x] <= x, and parent[x] only ever decreases; so a root (parent[x] == x) is the first vertex of its tree in this order.
 *   hook (one thread per face, edges (a, b) and (b, c)): two ends u, v start at the edge's vertices; while they differ the HIGHER end
 *     climbs to its parent, and when it is a root (parent[hi] == hi) it is hung below the other end with atomicCAS(&parent[hi], hi, lo).
 *     The CAS succeeds only on a true root; a failed CAS returns parent[hi] < hi, and the climb goes on FROM THAT RETURNED VALUE, never
 *     from a fresh plain load.  Every read of parent in this kernel is an agent-scope relaxed atomic load.  Two ends in one tree meet at
 *     their first common ancestor, so the root's own word -- where every walk of a big component would end -- is never read.  What is
 *     left in the lower end is an ancestor of both vertices, and they take it for their parent with atomicMin on their own words, which
 *     keeps the invariant under any race and touches no root (a vertex with a proper ancestor is none, and never will be again).
 *   Termination.  A step replaces the higher end by a value read from its parent word that differs from it, hence below it (a stale
 *     value is an earlier value of that word, also <= it), or by what the failed CAS returned, also below it; the other end stays.  The
 *     two positions in the order fall with every step, so one thread takes fewer than 2 V steps whatever the others do.  No thread waits
 *     for another thread's or workgroup's progress, no value is polled, there is no round count to bound: the hook is ONE launch.  A
 *     stale read costs a step, never correctness: every value ever read from parent[x] is an ancestor-or-self of x in the final forest.
 *   After the hook's launch has ended no root changes: roots [V] by a second launch in which vertex v walks to its root and moves its
 *     own parent along (pointer jumping without rounds: only thread v stores parent[v], each value an ancestor below the last; the walk
 *     falls with every step, so it ends however stale a read is).  Then each tree's smallest vertex INDEX by an integer atomicMin per
 *     run of vertices (exact, whatever the order), the ranks of the smallest vertices by a scan, ids by one gather: the ids do not
 *     depend on the key, on the order of the faces or on which thread won which compare-and-swap.
 *
 * Memory operations: vector atomics (atomicCAS, atomicMin, integer atomicAdd, the fp64 add of the volumes) and plain vector stores.
 *
 * Protocol.  label -> the caller reads counts_dev (C and the flag: the one synchronisation of a labelling) -> stats (and the caller's
 *   selection: [C]-sized work) -> filter_count -> the caller reads (V', F') and allocates -> filter_write.
 *
 * Workspace, in 8-byte words.  L(n) = n_1 + n_2 + ... with n_1 = ceil(n / 256), n_{k+1} = ceil(n_k / 256), down to the level of one
 * word; S(n) = 0 for n = 0 and G + L(G) with G = ceil(n / 256) otherwise (the counts of groups of 256 items and their scan).
 * perf_meshcc_workspace_bytes = 8 * ((V + S(V) + S(F) + 4) rounded up to an even number): two int32 arrays [V] (parent, then the
 * trees' smallest vertices and their ranks within their groups / the kept vertices' new indices; the roots), the vertices' and the faces' group counts, four
 * totals.  8 bytes per vertex and 1/32 byte per face, and the levels. */
#ifndef PERF_HIP_MESHCC_H
#define PERF_HIP_MESHCC_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_MESHCC_ABI_VERSION 1
#define PERF_MESHCC_MAX_VERTICES 1073741824 /* 2^30 */
#define PERF_MESHCC_MAX_FACES 274877906944  /* 2^38 */

int perf_meshcc_version(void);          /* == PERF_MESHCC_ABI_VERSION of the header the library was built from */

/* Bytes of the one workspace that serves label, filter_count and filter_write of a mesh of n_vertices and n_faces (a multiple of 16);
 * -1 with a reason: a negative count, n_vertices above PERF_MESHCC_MAX_VERTICES, n_faces above PERF_MESHCC_MAX_FACES. */
int64_t perf_meshcc_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* perf_meshcc_label: faces int32 [n_faces, 3] -> vertex_component int32 [n_vertices] and counts_dev [2] int64 ON THE DEVICE:
 * (C, the smallest index of a face with an index outside [0, n_vertices), or -1).  Such faces connect nothing; the caller refuses the
 * mesh when the flag is not -1.  faces may be NULL when n_faces is 0, vertex_component when n_vertices is 0.  workspace: 16-byte
 * aligned, >= workspace_bytes(n_vertices, n_faces). */
int perf_meshcc_label(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* vertex_component, int64_t* counts_dev,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* perf_meshcc_stats: faces_per_component int64 [C], vertices_per_component int32 [C] and, unless vertices is NULL, signed_volume
 * float64 [C] of the labelling vertex_component [n_vertices] with n_components = C components; vertices fp32 [n_vertices, 3].
 * signed_volume may be NULL when vertices is; with vertices NULL and signed_volume not, it is zeroed.  All outputs may be NULL when
 * n_components is 0.  Faces with an index outside [0, n_vertices) and ids outside [0, C) are skipped. */
int perf_meshcc_stats(const int32_t* faces, int64_t n_faces, const float* vertices, int64_t n_vertices, const int32_t* vertex_component,
                      int64_t n_components, int64_t* faces_per_component, int32_t* vertices_per_component, double* signed_volume,
                      void* stream);

/* perf_meshcc_filter_count: keep uint8 [n_components] (nonzero = kept) -> the kept vertices' new indices in the workspace and
 * counts_dev [2] int64 ON THE DEVICE: (V', F').  keep may be NULL when n_components is 0. */
int perf_meshcc_filter_count(const int32_t* faces, int64_t n_faces, const int32_t* vertex_component, int64_t n_vertices, const uint8_t* keep,
                             int64_t n_components, void* workspace, int64_t workspace_bytes, int64_t* counts_dev, void* stream);

/* perf_meshcc_filter_write: faces_out int32 [F', 3], kept_vertex_index int32 [V'] and, unless vertices is NULL, vertices_out fp32
 * [V', 3] of the SAME faces, labelling, keep and workspace perf_meshcc_filter_count was given (the stream's order puts it after the
 * count).  vertex_capacity / face_capacity: rows the arrays hold; capacities below the counted totals are refused: the call reads the
 * totals back from the workspace after the stream has drained, so it is not for stream capture.  Outputs may be NULL when their
 * capacity is 0; vertices_out must not be NULL when vertices is not and vertex_capacity > 0. */
int perf_meshcc_filter_write(const int32_t* faces, int64_t n_faces, const int32_t* vertex_component, int64_t n_vertices, const uint8_t* keep,
                             int64_t n_components, const float* vertices, const void* workspace, int64_t workspace_bytes, float* vertices_out,
                             int32_t* kept_vertex_index, int64_t vertex_capacity, int32_t* faces_out, int64_t face_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_MESHCC_H */
